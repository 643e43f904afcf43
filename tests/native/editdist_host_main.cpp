// Stand-alone driver of the edit distance's host code (ctcdecode_amd/csrc/editdist.h through tests/native/editdist_host.cpp), meant to
// be built with -fsanitize=address,undefined.  Every argument is a case file tests/test_editdist_host.py wrote -- the inputs and the
// outputs the numpy restatement expects -- and the twin's outputs are compared with them exactly; then pairs made here, every row a
// buffer of exactly its length, so that a read at or beyond a row's length is a sanitizer report, checked against closed forms and a
// full-matrix dynamic programme.  Prints "<checks> checks, <n> failures".
//
// Case file: int32 {B, R, L, Q, Lq, pairwise}, then x (B*R*L), x_lens (B*R), unless pairwise y (B*Q*Lq) and y_lens (B*Q), and the
// expectation: out (B*R*Q), status (B).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "editdist_host.cpp"

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

bool read_vec(std::FILE *f, std::vector<int32_t> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), 4, n, f) == n;
}

void run_file(const char *path) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) { expect(false, "case file opens"); return; }
  int32_t h[6];
  if (std::fread(h, 4, 6, f) != 6) { expect(false, "case header"); std::fclose(f); return; }
  const int B = h[0], R = h[1], L = h[2], Q = h[3], Lq = h[4];
  const bool pairwise = h[5] != 0;
  std::vector<int32_t> x, xl, y, yl, want, want_status;
  const bool ok = read_vec(f, x, (size_t)B * R * L) && read_vec(f, xl, (size_t)B * R) && read_vec(f, y, pairwise ? 0 : (size_t)B * Q * Lq) &&
                  read_vec(f, yl, pairwise ? 0 : (size_t)B * Q) && read_vec(f, want, (size_t)B * R * Q) && read_vec(f, want_status, (size_t)B);
  std::fclose(f);
  if (!ok) { expect(false, "case body"); return; }
  std::vector<int32_t> out((size_t)B * R * Q, 0x5A5A5A5A), status((size_t)B, 0);
  std::vector<int32_t> one(1, 0);  // (a general-mode y of no elements still needs an address)
  long long pairs = -1;
  const int rc = ctcedit_host_distance(x.data(), xl.data(), B, R, L, pairwise ? nullptr : (y.empty() ? one.data() : y.data()), pairwise ? nullptr : yl.data(), Q, Lq,
                                       out.data(), status.data(), &pairs);
  expect(rc == 0, "the twin takes the case", rc);
  expect(out == want, "distances == the restatement's");
  expect(status == want_status, "status == the restatement's");
  expect(pairs == (pairwise ? (long long)B * R * (R - 1) / 2 : (long long)B * R * Q), "the pair count", pairs);
}

int plain(const std::vector<int32_t> &a, const std::vector<int32_t> &b) {
  const size_t n = a.size(), m = b.size();
  std::vector<int> d((n + 1) * (m + 1));
  for (size_t i = 0; i <= n; ++i)
    for (size_t j = 0; j <= m; ++j) {
      int v;
      if (i == 0) v = (int)j;
      else if (j == 0) v = (int)i;
      else {
        v = d[(i - 1) * (m + 1) + j - 1] + (a[i - 1] != b[j - 1] ? 1 : 0);
        if (d[(i - 1) * (m + 1) + j] + 1 < v) v = d[(i - 1) * (m + 1) + j] + 1;
        if (d[i * (m + 1) + j - 1] + 1 < v) v = d[i * (m + 1) + j - 1] + 1;
      }
      d[i * (m + 1) + j] = v;
    }
  return d[n * (m + 1) + m];
}

int twin(const std::vector<int32_t> &a, const std::vector<int32_t> &b) {
  return ctcedit_host_pair(a.empty() ? nullptr : a.data(), (int)a.size(), b.empty() ? nullptr : b.data(), (int)b.size());
}

void run_made(Rng &r, int n, int m, int alphabet) {
  std::vector<int32_t> a((size_t)n), b((size_t)m);
  for (auto &v : a) v = r.below(alphabet);
  for (auto &v : b) v = r.below(alphabet);
  const int want = plain(a, b);
  expect(twin(a, b) == want, "random pair == the full-matrix programme", n, m);
  expect(twin(b, a) == want, "... with the roles swapped", n, m);
  expect(twin(a, a) == 0, "equal rows: 0", n);
  std::vector<int32_t> c(b);
  for (auto &v : c) v += alphabet;
  expect(twin(a, c) == (n > m ? n : m), "disjoint alphabets: max(m, n)", n, m);
  if (n <= m) {
    std::vector<int32_t> pre(b.begin(), b.begin() + n), suf(b.end() - n, b.end());
    expect(twin(pre, b) == m - n, "a prefix: m - n", n, m);
    expect(twin(b, suf) == m - n, "a suffix: m - n", n, m);
  }
}

}  // namespace

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) run_file(argv[i]);
  Rng r{20241021ull};
  const int ns[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 257, 513, 1025};
  for (int n : ns) {
    const int ms[] = {n, n + 1, n + 63, n + 64, n + 65};
    for (int m : ms) run_made(r, n, m, 2 + r.below(3));
  }
  run_made(r, 2048, 2048, 4);
  for (int rep = 0; rep < 200; ++rep) run_made(r, r.below(40), r.below(90), 2 + 2 * r.below(2));
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
