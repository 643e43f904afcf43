// Stand-alone driver of the host code of the greedy decode of live streams (ctcdecode_amd/csrc/greedy.h through
// tests/native/greedy_stream_host.cpp), meant to be built with -fsanitize=address,undefined.  Every argument is a scenario file
// tests/test_greedy_stream_host.py wrote -- the calls of a few streams and the outputs the slicing rule expects of each -- and the
// twin's outputs are compared with them bit for bit; then rows made here, cut into chunks at random: the calls' outputs concatenated
// must be what the one-shot routine (greedy_item_host) returns for the whole row.  Every buffer is sized exactly, so that an index that
// escapes its check is a sanitizer report.  Prints "<checks> checks, <n> failures".
//
// Scenario file: int32 {V, blank, log_input, dtype, streams, calls}, int64 first_frame per stream, then per call: int32 {B, Tc,
// has_seq_lens}, int32 stream index [B], uint8 eos [B], rows (B*Tc*V elements of 4 or 2 bytes), seq_lens (B, if any), and the
// expectation: tokens, starts (B*Tc int32 each), ends (B*(Tc+1) int32), label_scores (B*(Tc+1) floats), closed_lens (B int32), scores
// (B floats), lens (B int32).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "greedy_stream_host.cpp"

namespace {

long long checks = 0, failures = 0;
// (a comparison of no bytes never hands memcmp the NULL of an empty vector)
bool same_bytes(const void *a, const void *b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; }
void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
  ++checks;
  if (!ok) { ++failures; std::printf("FAIL %s (%lld, %lld)\n", what, a, b); }
}

struct Rng {
  unsigned long long s;
  unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
  int below(int n) { return n > 0 ? (int)(next() % (unsigned)n) : 0; }
};

template <typename T> bool read_vec(std::FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

void run_file(const char *path) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) { expect(false, "scenario file opens"); return; }
  int32_t h[6];
  if (std::fread(h, 4, 6, f) != 6) { expect(false, "scenario header"); std::fclose(f); return; }
  const int V = h[0], blank = h[1], log_input = h[2], dtype = h[3], n_streams = h[4], n_calls = h[5];
  std::vector<long long> first;
  if (!read_vec(f, first, (size_t)n_streams)) { expect(false, "first frames"); std::fclose(f); return; }
  std::vector<int32_t> recs((size_t)n_streams * 8);
  for (int s = 0; s < n_streams; ++s) expect(ctcgreedy_stream_host_init(recs.data() + (size_t)s * 8, first[(size_t)s]) == 0, "a stream is made");
  for (int j = 0; j < n_calls; ++j) {
    int32_t c[3];
    if (std::fread(c, 4, 3, f) != 3) { expect(false, "call header", j); break; }
    const int B = c[0], Tc = c[1];
    const size_t eb = dtype == 0 ? 4 : 2, n_bt = (size_t)B * Tc, n_bt1 = (size_t)B * (Tc + 1);
    std::vector<int32_t> idx, seq, want_tok, want_st, want_en, want_closed, want_len;
    std::vector<unsigned char> eos, rows;
    std::vector<float> want_ls, want_sc;
    const bool ok = read_vec(f, idx, (size_t)B) && read_vec(f, eos, (size_t)B) && read_vec(f, rows, n_bt * V * eb) && read_vec(f, seq, c[2] ? (size_t)B : 0) &&
                    read_vec(f, want_tok, n_bt) && read_vec(f, want_st, n_bt) && read_vec(f, want_en, n_bt1) && read_vec(f, want_ls, n_bt1) &&
                    read_vec(f, want_closed, (size_t)B) && read_vec(f, want_sc, (size_t)B) && read_vec(f, want_len, (size_t)B);
    if (!ok) { expect(false, "call body", j); break; }
    std::vector<int32_t> st8((size_t)B * 8), tok(n_bt, 0x5A5A5A5A), st(n_bt, 0x5A5A5A5A), en(n_bt1, 0x5A5A5A5A), closed((size_t)B, 0x5A5A5A5A), len((size_t)B, 0x5A5A5A5A);
    std::vector<float> ls(n_bt1, -123.0f), sc((size_t)B, -123.0f);
    for (int b = 0; b < B; ++b) std::memcpy(st8.data() + (size_t)b * 8, recs.data() + (size_t)idx[(size_t)b] * 8, 32);
    const int rc = ctcgreedy_stream_host_decode(st8.data(), eos.data(), rows.data(), dtype, c[2] ? seq.data() : nullptr, B, Tc, V, blank, log_input, tok.data(), st.data(),
                                                en.data(), ls.data(), closed.data(), sc.data(), len.data());
    for (int b = 0; b < B; ++b) std::memcpy(recs.data() + (size_t)idx[(size_t)b] * 8, st8.data() + (size_t)b * 8, 32);
    expect(rc == 0, "the twin takes the call", rc, j);
    expect(same_bytes(tok.data(), want_tok.data(), n_bt * 4), "tokens == the slicing rule's", j);
    expect(same_bytes(st.data(), want_st.data(), n_bt * 4), "starts == the slicing rule's", j);
    expect(same_bytes(en.data(), want_en.data(), n_bt1 * 4), "ends == the slicing rule's", j);
    expect(same_bytes(ls.data(), want_ls.data(), n_bt1 * 4), "label_scores == the slicing rule's, bit for bit", j);
    expect(same_bytes(closed.data(), want_closed.data(), (size_t)B * 4), "closed_lens == the slicing rule's", j);
    expect(same_bytes(sc.data(), want_sc.data(), (size_t)B * 4), "scores == the slicing rule's, bit for bit", j);
    expect(same_bytes(len.data(), want_len.data(), (size_t)B * 4), "lens == the slicing rule's", j);
  }
  std::fclose(f);
}

// one row of random log-probabilities (multiples of 1/8 and both zeros: ties are common), decoded at once and as a stream cut at random
void run_random(Rng &r, int T, int V, int blank, int first) {
  std::vector<float> lp((size_t)T * V);
  for (auto &v : lp) {
    const int k = r.below(16);
    v = k == 15 ? -0.0f : (k % 6 == 0 ? 0.0f : -0.125f * (float)(k % 6));
  }
  std::vector<ctcgreedy::FrameRec> rec((size_t)T);
  std::vector<int32_t> tok1((size_t)T, -1), st1((size_t)T, -1), en1((size_t)T, -1);
  std::vector<float> ls1((size_t)T, -123.0f);
  float sc1 = -123.0f;
  int32_t L = -1;
  ctcgreedy::greedy_item_host<0, 1>(lp.data(), nullptr, 0, T, V, blank, ctcmath::host_tables().w, rec.data(), tok1.data(), st1.data(), en1.data(), ls1.data(), &sc1, &L);
  std::vector<int32_t> tok, st, en;
  std::vector<float> ls;
  int32_t state[8];
  expect(ctcgreedy_stream_host_init(state, first) == 0, "a stream is made");
  float sc = 0.0f;
  int t = 0;
  bool ended = false;
  while (!ended) {
    const int Tc = r.below(T - t + 2), n = Tc > T - t ? T - t : Tc;  // (a chunk may claim a frame more than is left: seq_lens cuts it)
    const unsigned char eos = (t + n == T && r.below(2)) ? 1 : 0;
    const int32_t seq[1] = {n};
    std::vector<float> rows((size_t)Tc * V, -9.0f);
    if (n) std::memcpy(rows.data(), lp.data() + (size_t)t * V, (size_t)n * V * 4);
    std::vector<int32_t> ctok((size_t)Tc, -1), cst((size_t)Tc, -1), cen((size_t)Tc + 1, -1);
    std::vector<float> cls((size_t)Tc + 1, -123.0f);
    int32_t clen = -1, cclosed = -1;
    const int rc = ctcgreedy_stream_host_decode(state, &eos, rows.data(), 0, seq, 1, Tc, V, blank, 1, ctok.data(), cst.data(), cen.data(), cls.data(), &cclosed, &sc, &clen);
    expect(rc == 0, "the twin takes a random chunk", rc);
    if (rc != 0 || clen < 0 || clen > n || cclosed < 0 || cclosed > n + 1) { expect(false, "0 <= E <= n and 0 <= C <= n + 1", clen, cclosed); return; }
    bool tail = true;
    for (int i = clen; i < Tc; ++i) tail = tail && ctok[(size_t)i] == 0 && cst[(size_t)i] == 0;
    for (int i = cclosed; i <= Tc; ++i) tail = tail && cen[(size_t)i] == 0 && cls[(size_t)i] == 0.0f;
    expect(tail, "positions at or beyond the counts are 0");
    tok.insert(tok.end(), ctok.begin(), ctok.begin() + clen);
    st.insert(st.end(), cst.begin(), cst.begin() + clen);
    en.insert(en.end(), cen.begin(), cen.begin() + cclosed);
    ls.insert(ls.end(), cls.begin(), cls.begin() + cclosed);
    t += n;
    ended = eos != 0;
  }
  expect((int)tok.size() == L && (int)en.size() == L, "the calls return the row's labels and runs", (long long)tok.size(), L);
  if ((int)tok.size() != L || (int)en.size() != L) return;
  bool same = true;
  for (int i = 0; i < L; ++i)
    same = same && tok[(size_t)i] == tok1[(size_t)i] && st[(size_t)i] == st1[(size_t)i] + first && en[(size_t)i] == en1[(size_t)i] + first &&
           std::memcmp(&ls[(size_t)i], &ls1[(size_t)i], 4) == 0;
  expect(same, "the calls concatenated == the one-shot decode of the row, bit for bit");
  expect(std::memcmp(&sc, &sc1, 4) == 0, "the last call's score == the one-shot score, bit for bit");
  long long info[5];
  ctcgreedy_stream_host_info(state, info);
  expect(info[0] == T && info[1] == L && info[2] == L && info[3] == 0 && info[4] == 1, "the record counts the row", info[0], info[1]);
}

}  // namespace

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) run_file(argv[i]);
  Rng r{20261021ull};
  const int Ts[] = {0, 1, 2, 3, 15, 64, 65, 130};
  for (int T : Ts)
    for (int rep = 0; rep < 8; ++rep) {
      const int V = 1 + r.below(5);
      run_random(r, T, V, r.below(V), rep % 2 ? 0 : r.below(1000));
    }
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
