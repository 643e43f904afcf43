// Stand-alone driver of the edit operations' host code (ctcdecode_amd/csrc/editops.h through tests/native/editops_host.cpp), meant to be
// built with -fsanitize=address,undefined.  Every argument is a case file tests/test_editops_host.py wrote -- the inputs and the outputs
// the restatement expects -- and the twin's outputs are compared with them exactly; then pairs made here, every tensor a buffer of
// exactly its size and the back-pointer slot (inside the twin) of exactly ops_slot_bytes, so that a word read or stored outside a row
// or the slot is a sanitizer report, checked against a full-matrix programme over (D, S) tuples.  Prints "<checks> checks, <n> failures".
//
// Case file: int32 {B, R, L, Q, Lq, mode}, mode 0: counts, 1: counts pairwise, 2: align; then x (B*R*L), x_lens (B*R), unless pairwise
// y (B*Q*Lq) and y_lens (B*Q), and the expectation: counts (B*R*Q*4), for mode 2 x_to_y (B*R*Q*L) and y_to_x (B*R*Q*Lq), status (B).
#include <cstdio>
#include <utility>
#include <vector>

#include "editops_host.cpp"

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
  const int B = h[0], R = h[1], L = h[2], Q = h[3], Lq = h[4], mode = h[5];
  const bool pairwise = mode == 1, maps = mode == 2;
  const size_t P = (size_t)B * R * Q;
  std::vector<int32_t> x, xl, y, yl, want, want_xm, want_ym, want_status;
  const bool ok = read_vec(f, x, (size_t)B * R * L) && read_vec(f, xl, (size_t)B * R) && read_vec(f, y, pairwise ? 0 : (size_t)B * Q * Lq) &&
                  read_vec(f, yl, pairwise ? 0 : (size_t)B * Q) && read_vec(f, want, P * 4) && read_vec(f, want_xm, maps ? P * L : 0) &&
                  read_vec(f, want_ym, maps ? P * Lq : 0) && read_vec(f, want_status, (size_t)B);
  std::fclose(f);
  if (!ok) { expect(false, "case body"); return; }
  std::vector<int32_t> out(P * 4, 0x5A5A5A5A), status((size_t)B, 0), xm(maps ? P * L : 0, 0x5A5A5A5A), ym(maps ? P * Lq : 0, 0x5A5A5A5A);
  std::vector<int32_t> one(1, 0);  // (a general-mode y of no elements still needs an address)
  if (maps) {
    long long sb = -1;
    const int rc = ctcedit_host_align(x.data(), xl.data(), B, R, L, y.empty() ? one.data() : y.data(), yl.data(), Q, Lq, xm.data(), ym.data(), out.data(),
                                      status.data(), 0, 0xA5, &sb);
    expect(rc == 0, "the twin takes the case", rc);
    expect(sb == ctcedit_host_slot_bytes(L, Lq), "the slot size", sb);
    expect(xm == want_xm, "x_to_y == the restatement's");
    expect(ym == want_ym, "y_to_x == the restatement's");
  } else {
    long long pairs = -1;
    const int rc = ctcedit_host_counts(x.data(), xl.data(), B, R, L, pairwise ? nullptr : (y.empty() ? one.data() : y.data()), pairwise ? nullptr : yl.data(), Q, Lq,
                                       out.data(), status.data(), &pairs);
    expect(rc == 0, "the twin takes the case", rc);
    expect(pairs == (pairwise ? (long long)B * R * (R - 1) / 2 : (long long)B * R * Q), "the pair count", pairs);
  }
  expect(out == want, "counts == the restatement's");
  expect(status == want_status, "status == the restatement's");
}

// the definition over tuples, the whole matrix kept, and the walk's three rules
typedef std::pair<int, int> Key;
void plain(const std::vector<int32_t> &x, const std::vector<int32_t> &y, int32_t cnt[4], std::vector<int32_t> &xm, std::vector<int32_t> &ym) {
  const size_t n = x.size(), m = y.size(), w = m + 1;
  std::vector<Key> K((n + 1) * w);
  auto add = [](Key k, int d, int s) { return Key(k.first + d, k.second + s); };
  for (size_t i = 0; i <= n; ++i)
    for (size_t j = 0; j <= m; ++j) {
      if (i == 0) { K[j] = Key((int)j, 0); continue; }
      if (j == 0) { K[i * w] = Key((int)i, 0); continue; }
      const int ne = x[i - 1] != y[j - 1];
      Key v = add(K[(i - 1) * w + j - 1], ne, ne);
      if (add(K[(i - 1) * w + j], 1, 0) < v) v = add(K[(i - 1) * w + j], 1, 0);
      if (add(K[i * w + j - 1], 1, 0) < v) v = add(K[i * w + j - 1], 1, 0);
      K[i * w + j] = v;
    }
  xm.assign(n, -1);
  ym.assign(m, -1);
  size_t i = n, j = m;
  while (i > 0 || j > 0) {
    const int ne = i > 0 && j > 0 && x[i - 1] != y[j - 1];
    if (i > 0 && j > 0 && add(K[(i - 1) * w + j - 1], ne, ne) == K[i * w + j]) {
      xm[i - 1] = (int32_t)(j - 1), ym[j - 1] = (int32_t)(i - 1);
      --i, --j;
    } else if (i > 0 && add(K[(i - 1) * w + j], 1, 0) == K[i * w + j]) {
      --i;
    } else {
      --j;
    }
  }
  const int D = K[n * w + m].first, S = K[n * w + m].second;
  cnt[3] = (D - S + (int)n - (int)m) / 2, cnt[2] = (D - S - (int)n + (int)m) / 2, cnt[1] = S, cnt[0] = (int)n - S - cnt[3];
}

void run_pair(const std::vector<int32_t> &x, const std::vector<int32_t> &y, const char *what) {
  int32_t want[4];
  std::vector<int32_t> want_xm, want_ym;
  plain(x, y, want, want_xm, want_ym);
  const int lx = (int)x.size(), ly = (int)y.size();
  std::vector<int32_t> xl(1, lx), yl(1, ly), xm(x.size(), 0x5A5A5A5A), ym(y.size(), 0x5A5A5A5A), cnt(4, 0x5A5A5A5A), c2(4, 0x5A5A5A5A), one(1, 0);
  long long sb = -1, pairs = -1;
  int rc = ctcedit_host_align(x.empty() ? nullptr : x.data(), xl.data(), 1, 1, lx, y.empty() ? one.data() : y.data(), yl.data(), 1, ly, xm.empty() ? nullptr : xm.data(),
                              ym.empty() ? nullptr : ym.data(), cnt.data(), nullptr, 0, 0x5A, &sb);
  expect(rc == 0, what, lx, ly);
  expect(xm == want_xm && ym == want_ym, "maps == the full-matrix programme's", lx, ly);
  expect(cnt[0] == want[0] && cnt[1] == want[1] && cnt[2] == want[2] && cnt[3] == want[3], "align's counts", lx, ly);
  rc = ctcedit_host_counts(x.empty() ? nullptr : x.data(), xl.data(), 1, 1, lx, y.empty() ? one.data() : y.data(), yl.data(), 1, ly, c2.data(), nullptr, &pairs);
  expect(rc == 0 && c2 == cnt, "the counts entry == align's counts", lx, ly);
}

void run_made(Rng &r, int n, int m, int alphabet) {
  std::vector<int32_t> a((size_t)n), b((size_t)m);
  for (auto &v : a) v = r.below(alphabet);
  for (auto &v : b) v = r.below(alphabet);
  run_pair(a, b, "random pair");
  run_pair(b, a, "... with the roles swapped");
  run_pair(a, a, "equal rows");
}

}  // namespace

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) run_file(argv[i]);
  Rng r{20261021ull};
  const int ns[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 257, 513};
  for (int n : ns) {
    const int ms[] = {n, n + 1, n + 63, n + 64, n + 65};
    for (int m : ms) run_made(r, n, m, 2 + r.below(3));
  }
  run_made(r, 1025, 1100, 2);
  for (int rep = 0; rep < 200; ++rep) run_made(r, r.below(40), r.below(90), 2 + 2 * r.below(2));
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
