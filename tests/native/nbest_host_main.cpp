// Stand-alone driver of the n-best expansion's host code (ctcdecode_amd/csrc/nbest.h), meant to be built with
// -fsanitize=address,undefined: random tries, the chain whose owners cross every entry, short items, and malformed records, every
// buffer sized exactly so that an index that escapes its checks is a sanitizer report.  Prints "<checks> checks, <n> failures".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ctcdecode_amd/csrc/nbest.h"

namespace {

struct Rng {
  unsigned long long s;
  unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
  int below(int n) { return n > 0 ? (int)(next() % (unsigned)n) : 0; }
};

struct Records {
  int K = 0, T = 0;
  std::vector<int32_t> hdr, ent;
  std::vector<uint32_t> lab;
};

// one item: nres random sequences in trie order, rows a random permutation; `first` labels of padding in front of the item's own
Records random_item(Rng &r, int K, int T, int nres, int first) {
  Records x;
  x.K = K; x.T = T;
  x.hdr.assign(4, 0);
  x.ent.assign((size_t)K * 4, 0);
  for (int i = 0; i < first; ++i) x.lab.push_back(0xDEAD0000u + (unsigned)i);
  std::vector<int> rows(nres);
  for (int i = 0; i < nres; ++i) rows[i] = i;
  for (int i = nres - 1; i > 0; --i) std::swap(rows[i], rows[r.below(i + 1)]);
  int prev = 0;
  for (int j = 0; j < nres; ++j) {
    const int lcp = j == 0 ? 0 : r.below(prev + 1);
    const int dep = lcp + r.below(T - lcp + 1);
    int32_t *e = &x.ent[(size_t)j * 4];
    e[0] = rows[j]; e[1] = lcp; e[2] = dep; e[3] = (int32_t)x.lab.size();
    for (int q = lcp; q < dep; ++q) x.lab.push_back((unsigned)(1 + r.below(60000)) | ((unsigned)r.below(65536) << 16));
    prev = dep;
  }
  x.hdr[0] = nres; x.hdr[1] = (int32_t)x.lab.size() - first; x.hdr[2] = first;
  if (x.lab.empty()) x.lab.push_back(0);  // (a non-null pointer; n_labels stays 0)
  return x;
}

long long checks = 0, failures = 0;
void expect(bool ok, const char *what, int a = 0, int b = 0) {
  ++checks;
  if (!ok) { ++failures; std::printf("FAIL %s (%d, %d)\n", what, a, b); }
}

// both n-best methods against the slices of the full expansion, and their zero fill
void check_well_formed(const Records &x, int n, const char *what) {
  const int K = x.K, T = x.T;
  const unsigned long long nl = (unsigned long long)x.hdr[2] + (unsigned long long)x.hdr[1];
  std::vector<int32_t> ftok((size_t)K * T, -1), fts((size_t)K * T, -1);
  ctcbeam::expand_item_host(x.hdr.data(), x.ent.data(), x.lab.data(), 0, K, T, ftok.data(), fts.data());
  for (int method = 0; method < 2; ++method) {
    std::vector<int32_t> tok((size_t)n * T, -1), ts((size_t)n * T, -1);
    std::vector<unsigned char> ok((size_t)n, 9);
    const int st = method == 0 ? ctcnbest::expand_item_nbest_host(x.hdr.data(), x.ent.data(), x.lab.data(), nl, 0, K, T, n, tok.data(), ts.data(), ok.data())
                               : ctcnbest::rows_by_segments_host(x.hdr.data(), x.ent.data(), x.lab.data(), nl, 0, K, T, n, tok.data(), ts.data(), ok.data());
    expect(st == 0, what, method, st);
    bool same = true;
    for (size_t i = 0; i < (size_t)n * T; ++i) same = same && tok[i] == ftok[i] && ts[i] == fts[i];
    expect(same, what, method, n);
    int have = 0;
    for (int p = 0; p < n; ++p) have += ok[(size_t)p];
    expect(have == (x.hdr[0] < n ? x.hdr[0] : n), "rows with a result", have, n);
  }
}

// a malformed record: both methods report it, write every row (no word of the outputs keeps its fill) and stay inside their buffers
void check_malformed(const Records &x, unsigned long long nl, int n, const char *what) {
  const int K = x.K, T = x.T;
  for (int method = 0; method < 2; ++method) {
    std::vector<int32_t> tok((size_t)n * T, -1), ts((size_t)n * T, -1);
    std::vector<unsigned char> ok((size_t)n, 9);
    const int st = method == 0 ? ctcnbest::expand_item_nbest_host(x.hdr.data(), x.ent.data(), x.lab.data(), nl, 0, K, T, n, tok.data(), ts.data(), ok.data())
                               : ctcnbest::rows_by_segments_host(x.hdr.data(), x.ent.data(), x.lab.data(), nl, 0, K, T, n, tok.data(), ts.data(), ok.data());
    expect(st == ctcnbest::NBEST_BAD_RECORD, what, method, st);
    bool written = true;
    for (size_t i = 0; i < (size_t)n * T; ++i) written = written && tok[i] != -1 && ts[i] != -1;
    expect(written, "every row written", method, n);
    for (int p = 0; p < n; ++p)
      if (!ok[(size_t)p]) {
        bool zero = true;
        for (int q = 0; q < T; ++q) zero = zero && tok[(size_t)p * T + q] == 0 && ts[(size_t)p * T + q] == 0;
        expect(zero, "a row without a well-formed result is zero", method, p);
      }
  }
}

}  // namespace

int main() {
  Rng r{20240607ull};
  const int Ts[] = {1, 3, 64, 67};
  const int Ks[] = {1, 2, 8, 16, 70};
  for (int T : Ts)
    for (int K : Ks)
      for (int rep = 0; rep < 6; ++rep) {
        const int nres = rep == 0 ? 0 : (rep == 1 ? K : 1 + r.below(K));
        const Records x = random_item(r, K, T, nres, rep % 2 ? 5 : 0);
        const int ns[] = {1, K > 1 ? K - 1 : 1, K};
        for (int n : ns) check_well_formed(x, n, "random trie");
      }
  {  // the chain: entry j shares j labels with its predecessor and adds one; the last entry is row 0 and every entry owns one of its labels
    Records x;
    x.K = 66; x.T = 67;
    x.hdr.assign(4, 0);
    x.ent.assign((size_t)x.K * 4, 0);
    for (int j = 0; j < x.K; ++j) {
      int32_t *e = &x.ent[(size_t)j * 4];
      e[0] = x.K - 1 - j; e[1] = j; e[2] = j + 1; e[3] = j;
      x.lab.push_back((unsigned)(j + 1) | ((unsigned)(2 * j) << 16));
    }
    x.hdr[0] = x.K; x.hdr[1] = x.K; x.hdr[2] = 0;
    check_well_formed(x, 1, "chain");
    check_well_formed(x, 65, "chain");
    check_well_formed(x, 66, "chain");
  }
  for (int rep = 0; rep < 40; ++rep) {  // malformed records
    const int K = 8, T = 16;
    Records x = random_item(r, K, T, K, 3);
    const unsigned long long nl = x.lab.size();
    const int j = r.below(K);
    int32_t *e = &x.ent[(size_t)j * 4];
    switch (rep % 8) {
      case 0: e[3] = (int32_t)nl + 7; e[2] = e[1] + 1; break;  // labels beyond the buffer
      case 1: e[3] = 0; e[2] = e[1] + 1; break;                // labels in front of the item's own
      case 2: e[0] = K; break;                                // row index at the beam width
      case 3: e[0] = -1; break;                               // ... and below zero
      case 4: e[2] = T + 1; break;                            // longer than a row
      case 5: e[1] = e[2] + 1; if (j == 0) e[2] = -1; break;  // shares more than it has
      case 6: x.hdr[0] = K + 1; break;                        // more results than entries
      default: x.hdr[1] = (int32_t)nl; break;                 // the item's range beyond the buffer (first + total > n_labels)
    }
    const int ns[] = {1, K - 1, K};
    for (int n : ns) check_malformed(x, nl, n, "malformed record");
  }
  {  // a row claimed twice
    Records x = random_item(r, 8, 16, 8, 0);
    x.ent[4] = x.ent[0];
    check_malformed(x, x.lab.size(), 8, "row claimed twice");
  }
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
