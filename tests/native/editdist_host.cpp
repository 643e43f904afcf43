// Host twin of the edit distance (ctcdecode_amd/csrc/editdist.h): the routines the kernel of editdist.hip compiles -- the cell update,
// a lane's start and step, the result's lane and column, the step count, the class function, the pair enumeration and the length check
// -- run with 64 simulated lanes, one after the other, behind a C ABI.  Test infrastructure only.
#include "../../ctcdecode_amd/csrc/editdist.h"

// The whole contract of ctcd_edit_distance on host arrays (y == NULL: pairwise mode).  Returns 0, -1 for bad arguments, -2 beyond the
// limit; *pairs: the distances computed.  Rows are read through exactly the checked lengths: in the stand-alone driver, whose buffers
// are sized exactly, an index that escapes is a sanitizer report.
extern "C" int ctcedit_host_distance(const int32_t *x, const int32_t *x_lens, int B, int R, int L, const int32_t *y, const int32_t *y_lens, int Q, int Lq,
                                     int32_t *out, int32_t *status, long long *pairs) {
  const bool pairwise = y == nullptr;
  if (pairwise) Q = R, Lq = L;
  if (B < 0 || R < 0 || L < 0 || Q < 0 || Lq < 0 || !pairs) return -1;
  *pairs = 0;
  if (B == 0 || R == 0 || Q == 0) return 0;
  if (!x_lens || !out || (!x && L > 0) || (!pairwise && !y_lens)) return -1;
  if ((L < Lq ? L : Lq) > ctcedit::kEditMaxStrip) return -2;
  return ctcedit::edit_distance_host(x, x_lens, B, R, L, y, y_lens, Q, Lq, out, status, pairs);
}
// one pair of plain sequences
extern "C" int ctcedit_host_pair(const int32_t *a, int la, const int32_t *b, int lb) { return ctcedit::pair_host(a, la, b, lb); }
extern "C" int ctcedit_host_class(int n) { return ctcedit::strip_class(n); }
extern "C" int ctcedit_host_num_classes(int32_t *classes) {
  for (int i = 0; i < ctcedit::kEditNumClasses; ++i) classes[i] = ctcedit::kEditClasses[i];
  return ctcedit::kEditNumClasses;
}
extern "C" int ctcedit_host_max_strip() { return ctcedit::kEditMaxStrip; }
extern "C" void ctcedit_host_pair_of(long long w, int R, int Q, int pairwise, int32_t *bij) {
  const ctcedit::Pair p = ctcedit::pair_of(w, R, Q, pairwise != 0);
  bij[0] = p.b; bij[1] = p.i; bij[2] = p.j;
}
extern "C" long long ctcedit_host_pairs_per_item(int R, int Q, int pairwise) { return ctcedit::pairs_per_item(R, Q, pairwise != 0); }
// {result lane, result column, steps} of a strip of n tokens against m streamed ones in class C
extern "C" void ctcedit_host_result_at(int m, int n, int C, int32_t *lcs) {
  lcs[0] = ctcedit::result_lane(n, C); lcs[1] = ctcedit::result_col(n, C); lcs[2] = ctcedit::sweep_steps(m, n, C);
}
extern "C" int ctcedit_host_cell(int up, int left, int diag, int32_t a, int32_t b) { return ctcedit::cell_update(up, left, diag, a, b); }
