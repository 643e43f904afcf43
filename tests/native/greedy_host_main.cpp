// Stand-alone driver of the greedy decode's host code (ctcdecode_amd/csrc/greedy.h through tests/native/greedy_host.cpp), meant to be
// built with -fsanitize=address,undefined.  Every argument is a case file tests/test_greedy_host.py wrote -- the inputs and the outputs
// the numpy restatement expects -- and the twin's outputs are compared with them bit for bit; then rows made here, whose results are
// checked against properties that need no second implementation.  Every buffer is sized exactly, so that an index that escapes its
// check is a sanitizer report.  Prints "<checks> checks, <n> failures".
//
// Case file: int32 {B, T, V, blank, log_input, dtype, has_seq_lens}, then rows (B*T*V elements of 4 or 2 bytes), seq_lens (B, if any),
// and the expectation: tokens, starts, ends (B*T int32 each), label_scores (B*T floats), scores (B floats), lens (B int32).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "greedy_host.cpp"

namespace {

long long checks = 0, failures = 0;
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
  if (!f) { expect(false, "case file opens"); return; }
  int32_t h[7];
  if (std::fread(h, 4, 7, f) != 7) { expect(false, "case header"); std::fclose(f); return; }
  const int B = h[0], T = h[1], V = h[2], blank = h[3], log_input = h[4], dtype = h[5];
  const size_t eb = dtype == 0 ? 4 : 2, n_bt = (size_t)B * T;
  std::vector<unsigned char> rows;
  std::vector<int32_t> seq, want_tok, want_st, want_en, want_len;
  std::vector<float> want_ls, want_sc;
  const bool ok = read_vec(f, rows, n_bt * V * eb) && read_vec(f, seq, h[6] ? (size_t)B : 0) && read_vec(f, want_tok, n_bt) && read_vec(f, want_st, n_bt) &&
                  read_vec(f, want_en, n_bt) && read_vec(f, want_ls, n_bt) && read_vec(f, want_sc, (size_t)B) && read_vec(f, want_len, (size_t)B);
  std::fclose(f);
  if (!ok) { expect(false, "case body"); return; }
  std::vector<int32_t> tok(n_bt, 0x5A5A5A5A), st(n_bt, 0x5A5A5A5A), en(n_bt, 0x5A5A5A5A), len((size_t)B, 0x5A5A5A5A);
  std::vector<float> ls(n_bt, -123.0f), sc((size_t)B, -123.0f);
  const int rc = ctcgreedy_host_decode(rows.data(), dtype, h[6] ? seq.data() : nullptr, B, T, V, blank, log_input, tok.data(), st.data(), en.data(), ls.data(),
                                       sc.data(), len.data());
  expect(rc == 0, "the twin takes the case", rc);
  expect(std::memcmp(tok.data(), want_tok.data(), n_bt * 4) == 0, "tokens == the restatement's");
  expect(std::memcmp(st.data(), want_st.data(), n_bt * 4) == 0, "starts == the restatement's");
  expect(std::memcmp(en.data(), want_en.data(), n_bt * 4) == 0, "ends == the restatement's");
  expect(std::memcmp(ls.data(), want_ls.data(), n_bt * 4) == 0, "label_scores == the restatement's, bit for bit");
  expect(std::memcmp(sc.data(), want_sc.data(), (size_t)B * 4) == 0, "scores == the restatement's, bit for bit");
  expect(std::memcmp(len.data(), want_len.data(), (size_t)B * 4) == 0, "lens == the restatement's");
}

// one item of random log-probabilities (multiples of 1/8: additions are exact, ties are common): the spans are ordered runs of the
// label they name, every frame outside them is blank or repeats nothing new, the score is the sum of the frames' greatest values
void run_random(Rng &r, int T, int V, int blank) {
  std::vector<float> lp((size_t)T * V);
  for (auto &v : lp) v = -0.125f * (float)r.below(16);
  const int32_t n_arr[1] = {T + 1 - r.below(3)};
  const int n = n_arr[0] > T ? T : (n_arr[0] < 0 ? 0 : n_arr[0]);
  std::vector<int32_t> tok((size_t)T, -1), st((size_t)T, -1), en((size_t)T, -1), len(1, -1);
  std::vector<float> ls((size_t)T, -123.0f), sc(1, -123.0f);
  const int rc = ctcgreedy_host_decode(lp.data(), 0, n_arr, 1, T, V, blank, 1, tok.data(), st.data(), en.data(), ls.data(), sc.data(), len.data());
  expect(rc == 0, "the twin takes random rows", rc);
  const int L = len[0];
  expect(0 <= L && L <= n, "0 <= L <= n", L, n);
  if (L < 0 || L > n) return;
  bool tail = true;
  for (int i = L; i < T; ++i) tail = tail && tok[(size_t)i] == 0 && st[(size_t)i] == 0 && en[(size_t)i] == 0 && ls[(size_t)i] == 0.0f;
  expect(tail, "positions at or beyond L are 0");
  float sum = 0.0f;
  std::vector<int> lab((size_t)n);
  for (int t = 0; t < n; ++t) {
    int best = 0;
    for (int c = 1; c < V; ++c)
      if (lp[(size_t)t * V + c] > lp[(size_t)t * V + best]) best = c;
    lab[(size_t)t] = best;
    sum = t == 0 ? lp[(size_t)t * V + best] : sum + lp[(size_t)t * V + best];
  }
  expect(n == 0 ? sc[0] == 0.0f : std::memcmp(&sum, &sc[0], 4) == 0, "the score is the sum of the frames' greatest values");
  bool shape = true;
  for (int i = 0; i < L && shape; ++i) {
    shape = 0 <= st[(size_t)i] && st[(size_t)i] <= en[(size_t)i] && en[(size_t)i] < n && tok[(size_t)i] != blank && (i == 0 || st[(size_t)i] > en[(size_t)i - 1]);
    float m = -1e30f;
    for (int t = st[(size_t)i]; shape && t <= en[(size_t)i]; ++t) {
      shape = lab[(size_t)t] == tok[(size_t)i];
      m = lp[(size_t)t * V + tok[(size_t)i]] > m ? lp[(size_t)t * V + tok[(size_t)i]] : m;
    }
    shape = shape && m == ls[(size_t)i];
  }
  expect(shape, "spans are ordered runs of their label, with the run's greatest value");
}

}  // namespace

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) run_file(argv[i]);
  Rng r{20241021ull};
  const int Ts[] = {0, 1, 2, 3, 15, 64, 65, 130};
  for (int T : Ts)
    for (int rep = 0; rep < 6; ++rep) {
      const int V = 1 + r.below(6);
      run_random(r, T, V, r.below(V));
    }
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
