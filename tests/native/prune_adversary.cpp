// Adversarial rows for the vocabulary prune's std::sort replay (prepass.hip prune_resolve_kernel ->
// stl_emul.h sort_prefix_parallel), and a certificate of what such a row makes the replay do.  TEST INFRASTRUCTURE ONLY.
//
//   * Generator: McIlroy's "A Killer Adversary for Quicksort" (1999), played against the live std::sort under the descending
//     comparator the prune uses (as tests/native/stl_emul_check.cpp plays it): integer ranks, one per label, larger = better.
//   * Certificate: the introsort recursion of one row walked with the SERIAL primitives of stl_emul.h in the order the workgroup
//     form takes it -- ranges longer than big_cut one at a time from a stack (a "workgroup round" each), the rest in rounds of one
//     range per thread ("thread rounds"), ranges that start at or beyond top_n dropped, the heap sort wherever a range's depth
//     budget 2 * floor_lg(V) is spent -- and what it met on the way.  Nothing of the workgroup forms themselves runs here: the
//     certificate says which of their branches a row reaches on the device, not whether they are right.
#include "../../ctcdecode_amd/csrc/stl_emul.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

namespace {

struct Adversary {
  std::vector<int> val;
  int gas, nsolid = 0, candidate = 0;
  explicit Adversary(int n) : val(n, n), gas(n) {}
  bool less(int x, int y) {
    if (val[x] == gas && val[y] == gas) {
      if (x == candidate) val[x] = nsolid++; else val[y] = nsolid++;
    }
    if (val[x] == gas) candidate = x; else if (val[y] == gas) candidate = y;
    return val[x] < val[y];
  }
};

// the order of the doubles the reference compares (prepass.hip prune_key): -0 == +0, NaN below every number
uint32_t key_of_float(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 1u;
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct Range { int first, last, depth; };

}  // namespace

extern "C" {

// ranks[n]: the killer of std::sort(descending) on n elements in index order (big_left != 0: the long side of every partition starts
// at place 0; 0: the ascending killer, whose long side lies on the right), every rank divided by `fold` (ties in groups of `fold`).
int ctcadv_killer(int n, int big_left, int fold, int32_t *ranks) {
  if (n < 0 || fold < 1 || !ranks) return 0;
  Adversary adv(n);
  std::vector<int> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  std::sort(idx.begin(), idx.end(), [&](int a, int b) { return big_left ? adv.less(b, a) : adv.less(a, b); });
  for (int &v : adv.val) if (v == adv.gas) v = adv.nsolid++;
  for (int i = 0; i < n; ++i) ranks[i] = adv.val[i] / fold;
  return 1;
}

// out[12]: 0 workgroup rounds | 1 thread rounds | 2 heap sorts on ranges > big_cut | 3 the longest of them | 4 heap sorts on ranges
// <= big_cut | 5 the longest of them | 6 the largest number of pending long ranges (slots of bstack in use) | 7 the sorted row ties
// across places top_n - 1 | top_n | 8 ranges dropped because they start at or beyond top_n | 9 the longest of them | 10 the most
// ranges one thread round holds | 11 the walk's first min(top_n, n) places equal std::sort's (1; 0 = the walk itself is wrong)
int ctcadv_certificate(const float *row, int n, int top_n, int big_cut, int32_t *out) {
  if (!row || !out || n < 0 || n > 65535 || top_n < 1 || big_cut < 16) return 0;
  for (int i = 0; i < 12; ++i) out[i] = 0;
  typedef unsigned long long Pair;  // (key, label) as the replay holds them
  std::vector<Pair> v(n), want(n);
  for (int i = 0; i < n; ++i) v[i] = ((Pair)key_of_float(row[i]) << 32) | (unsigned)i;
  want = v;
  auto before = [](Pair a, Pair b) { return (uint32_t)(a >> 32) > (uint32_t)(b >> 32); };
  std::sort(want.begin(), want.end(), before);
  const int limit = top_n, upto = std::min(n, limit);
  out[7] = top_n < n && (uint32_t)(want[top_n - 1] >> 32) == (uint32_t)(want[top_n] >> 32);
  std::vector<int> stack(3 * (2 * stlemu::floor_lg(n > 0 ? n : 1) + 4));
  if (n <= 16) {
    stlemu::sort(v.data(), 0, n, before, stack.data());
  } else {
    std::vector<Range> big, cur, nxt, fin;
    big.push_back({0, n, 2 * stlemu::floor_lg(n)});
    out[6] = 1;
    auto heap = [&](const Range &r, int count_at) {
      stlemu::heap_select(v.data(), r.first, r.last, r.last, before);
      stlemu::heap_sort_down(v.data(), r.first, r.last, before);
      ++out[count_at];
      out[count_at + 1] = std::max(out[count_at + 1], r.last - r.first);
    };
    auto children = [&](const Range &r, int cut, std::vector<Range> &pending) {
      for (int side = 0; side < 2; ++side) {
        const int a = side ? cut : r.first, e = side ? r.last : cut;
        if (a >= limit) {
          ++out[8];
          out[9] = std::max(out[9], e - a);
          continue;
        }
        if (e - a > 16) pending.push_back({a, e, r.depth - 1});
        else if (e - a > 1) fin.push_back({a, e, 0});
      }
    };
    while (!big.empty()) {
      const Range r = big.back();
      big.pop_back();
      if (r.last - r.first <= big_cut) { cur.push_back(r); continue; }
      if (r.depth == 0) { heap(r, 2); continue; }
      ++out[0];
      children(r, stlemu::split_with_median_pivot(v.data(), r.first, r.last, before), big);
      out[6] = std::max(out[6], (int32_t)big.size());
    }
    while (!cur.empty()) {
      ++out[1];
      out[10] = std::max(out[10], (int32_t)cur.size());
      nxt.clear();
      for (const Range &r : cur) {
        if (r.depth == 0) { heap(r, 4); continue; }
        children(r, stlemu::split_with_median_pivot(v.data(), r.first, r.last, before), nxt);
      }
      cur.swap(nxt);
    }
    for (const Range &r : fin) stlemu::insertion_sort(v.data(), r.first, r.last, before);
  }
  out[11] = std::equal(v.begin(), v.begin() + upto, want.begin());
  return 1;
}

}  // extern "C"
