// Stand-alone driver of the forced alignment's host code (ctcdecode_amd/csrc/align.h through tests/native/align_host.cpp), meant to be
// built with -fsanitize=address,undefined.  Every argument is a case file tests/test_align_host.py wrote -- the inputs and the outputs
// the numpy restatement expects -- and the twin's outputs are compared with them bit for bit; then rows made here: out-of-range labels
// and lengths, and random rows whose score is re-added along the path their spans name.  Every buffer is sized exactly, so that an index
// that escapes its check is a sanitizer report.  Prints "<checks> checks, <n> failures".
//
// Case file: int32 {B, T, V, R, L_stride, blank, log_input, dtype, has_seq_lens}, then rows (B*T*V elements of 4 or 2 bytes), seq_lens
// (B, if any), tokens (B*R*L_stride), lens (B*R), and the expectation: start, end (B*R*L_stride each), scores (B*R floats), status (B).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "align_host.cpp"

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
  int32_t h[9];
  if (std::fread(h, 4, 9, f) != 9) { expect(false, "case header"); std::fclose(f); return; }
  const int B = h[0], T = h[1], V = h[2], R = h[3], Ls = h[4], blank = h[5], log_input = h[6], dtype = h[7];
  const size_t eb = dtype == 0 ? 4 : 2, n_rows = (size_t)B * T * V, n_tok = (size_t)B * R * Ls, n_hyp = (size_t)B * R;
  std::vector<unsigned char> rows;
  std::vector<int32_t> seq, tok, lens, want_st, want_en, want_status;
  std::vector<float> want_sc;
  bool ok = read_vec(f, rows, n_rows * eb) && read_vec(f, seq, h[8] ? (size_t)B : 0) && read_vec(f, tok, n_tok) && read_vec(f, lens, n_hyp) &&
            read_vec(f, want_st, n_tok) && read_vec(f, want_en, n_tok) && read_vec(f, want_sc, n_hyp) && read_vec(f, want_status, (size_t)B);
  std::fclose(f);
  if (!ok) { expect(false, "case body"); return; }
  std::vector<int32_t> st(n_tok, 0x5A5A5A5A), en(n_tok, 0x5A5A5A5A), status((size_t)B, 0);
  std::vector<float> sc(n_hyp, -123.0f);
  const int rc = ctcalign_host_align(rows.data(), dtype, h[8] ? seq.data() : nullptr, B, T, V, blank, log_input, tok.data(), lens.data(), R, Ls, st.data(), en.data(),
                                     sc.data(), status.data());
  expect(rc >= 0, "the twin takes the case", rc);
  expect(std::memcmp(st.data(), want_st.data(), n_tok * 4) == 0, "start == the restatement's");
  expect(std::memcmp(en.data(), want_en.data(), n_tok * 4) == 0, "end == the restatement's");
  expect(std::memcmp(sc.data(), want_sc.data(), n_hyp * 4) == 0, "scores == the restatement's, bit for bit");
  expect(std::memcmp(status.data(), want_status.data(), (size_t)B * 4) == 0, "status == the restatement's");
}

// one item of random log-probabilities (multiples of 1/8: additions are exact, ties are common) and random rows; the score of every
// aligned row must be the sum, in frame order, along the path its spans name
void run_random(Rng &r, int T, int V, int R, int Ls, int blank, bool with_inf) {
  std::vector<float> lp((size_t)T * V);
  for (auto &v : lp) v = -0.125f * (float)r.below(64);
  if (with_inf && T > 2)
    for (int c = 0; c < V; ++c)
      if (c != blank && r.below(3) == 0) lp[(size_t)(T / 2) * V + c] = ctcalign::neg_inf();
  std::vector<int32_t> tok((size_t)R * Ls, 0), lens((size_t)R, 0), st((size_t)R * Ls, -1), en((size_t)R * Ls, -1), status(1, 0);
  std::vector<float> sc((size_t)R, -123.0f);
  for (int p = 0; p < R; ++p) {
    const int L = r.below(Ls + 1);
    lens[(size_t)p] = L;
    for (int i = 0; i < L; ++i) {
      int c = r.below(V - 1);
      if (c >= blank) ++c;
      tok[(size_t)p * Ls + i] = (i > 0 && r.below(4) == 0) ? tok[(size_t)p * Ls + i - 1] : c;
    }
  }
  const int32_t n_arr[1] = {T - r.below(2)};
  const int n = n_arr[0] < 0 ? 0 : n_arr[0];
  const int rc = ctcalign_host_align(lp.data(), 0, n_arr, 1, T, V, blank, 1, tok.data(), lens.data(), R, Ls, st.data(), en.data(), sc.data(), status.data());
  expect(rc == 0 && status[0] == 0, "valid rows raise nothing", rc, status[0]);
  for (int p = 0; p < R; ++p) {
    const int L = lens[(size_t)p];
    const int32_t *s = st.data() + (size_t)p * Ls, *e = en.data() + (size_t)p * Ls, *y = tok.data() + (size_t)p * Ls;
    bool tail = true;
    for (int i = L; i < Ls; ++i) tail = tail && s[i] == 0 && e[i] == 0;
    expect(tail, "positions at or beyond the length are 0", p);
    if (!(sc[(size_t)p] > ctcalign::neg_inf()) || n == 0) {
      bool zero = true;
      for (int i = 0; i < L; ++i) zero = zero && s[i] == 0 && e[i] == 0;
      expect(zero, "a row that is not aligned has zero spans", p);
      continue;
    }
    bool shape = true;
    for (int i = 0; i < L; ++i) {
      shape = shape && 0 <= s[i] && s[i] <= e[i] && e[i] < n;
      if (i > 0) shape = shape && s[i] > e[i - 1] && (y[i] != y[i - 1] || s[i] > e[i - 1] + 1);
    }
    expect(shape, "spans are ordered, inside the item, with a blank between equal labels", p);
    if (!shape) continue;
    float sum = 0.0f;
    int i = 0;
    for (int t = 0; t < n; ++t) {
      while (i < L && t > e[i]) ++i;
      const int c = (i < L && t >= s[i]) ? y[i] : blank;
      const float v = lp[(size_t)t * V + c];
      sum = t == 0 ? v : v + sum;
    }
    expect(std::memcmp(&sum, &sc[(size_t)p], 4) == 0, "the score is the sum along the path the spans name", p);
  }
}

// rows with out-of-range labels and lengths between valid ones: zero outputs, score 0, the status raised, the valid rows untouched by it
void run_invalid(Rng &r) {
  const int T = 12, V = 5, R = 6, Ls = 7, blank = 1;
  std::vector<float> lp((size_t)2 * T * V);
  for (auto &v : lp) v = -0.25f * (float)(1 + r.below(16));
  std::vector<int32_t> tok((size_t)2 * R * Ls, 2), lens((size_t)2 * R, 3);
  auto row = [&](int b, int p) { return &tok[((size_t)b * R + p) * Ls]; };
  row(0, 1)[1] = V;            // a label = V
  row(0, 2)[0] = blank;        // a label = blank
  row(0, 3)[2] = -1;           // a negative label
  lens[4] = -1;                // a negative length
  lens[5] = Ls + 1;            // a length beyond the stride
  row(0, 0)[5] = 1 << 30;      // (beyond the row's length: never looked at)
  std::vector<int32_t> st((size_t)2 * R * Ls, -1), en((size_t)2 * R * Ls, -1), status(2, 0);
  std::vector<float> sc((size_t)2 * R, -123.0f);
  const int rc = ctcalign_host_align(lp.data(), 0, nullptr, 2, T, V, blank, 1, tok.data(), lens.data(), R, Ls, st.data(), en.data(), sc.data(), status.data());
  expect(rc == 5, "five invalid rows", rc);
  expect(status[0] == ctcalign::ALIGN_BAD_ROW && status[1] == 0, "the status of the item with invalid rows alone", status[0], status[1]);
  for (int p = 1; p < R; ++p) {
    bool zero = sc[(size_t)p] == 0.0f;
    for (int i = 0; i < Ls; ++i) zero = zero && st[(size_t)p * Ls + i] == 0 && en[(size_t)p * Ls + i] == 0;
    expect(zero, "an invalid row is zero with score 0", p);
  }
  expect(sc[0] > ctcalign::neg_inf() && en[2] >= st[2] && sc[(size_t)R] > ctcalign::neg_inf(), "the valid rows are aligned");
}

}  // namespace

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) run_file(argv[i]);
  Rng r{20241020ull};
  run_invalid(r);
  const int Ts[] = {1, 2, 3, 15, 16, 17, 40};
  for (int T : Ts)
    for (int rep = 0; rep < 6; ++rep) run_random(r, T, 2 + r.below(5), 5, T + (rep % 3) - 1 < 0 ? 0 : T + (rep % 3) - 1, 0, rep >= 4);
  for (int rep = 0; rep < 4; ++rep) run_random(r, 150, 4, 3, 140, 2, false);  // (S beyond 256: several words per frame)
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
