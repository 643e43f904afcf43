// Host twin of the CTC prefix scores (ctcdecode_amd/csrc/prefix.h): the routines the kernels of prefix.hip compile -- the (m, s) step,
// phi, the advance cell, the end score -- run sequentially for ONE prefix of one item behind a C ABI.  rows: the item's float32
// [T, V] rows; prob: they are probabilities; cols: [T, 2].  Test infrastructure only.
#define CTC_EXACT_MATH_HOST_TABLES
#include "../../ctcdecode_amd/csrc/prefix.h"

using namespace ctcprefix;
static const uint64_t *tbl() { return ctcmath::host_tables().w; }

extern "C" void ctcprefix_host_init(const float *rows, int prob, int n, int V, float *cols) {
  prob ? init_host<0, true>(rows, 0, n, V, 0, tbl(), cols) : init_host<0, false>(rows, 0, n, V, 0, tbl(), cols);
}
extern "C" void ctcprefix_host_advance(const float *rows, int prob, int n, int V, const float *pcols, int L, int last, int c, float *ccols) {
  prob ? advance_host<0, true>(rows, 0, n, V, 0, pcols, L, last, c, tbl(), ccols) : advance_host<0, false>(rows, 0, n, V, 0, pcols, L, last, c, tbl(), ccols);
}
// the valid candidates cands[0 .. C) of one prefix
extern "C" void ctcprefix_host_scores(const float *rows, int prob, int n, int V, const float *cols, int L, int last, const int32_t *cands, int C, float *out) {
  for (int k = 0; k < C; ++k)
    out[k] = prob ? score_host<0, true>(rows, 0, n, V, cols, L, last, cands[k], tbl()) : score_host<0, false>(rows, 0, n, V, cols, L, last, cands[k], tbl());
}
extern "C" float ctcprefix_host_eos(int n, const float *cols, int L) { return eos_host(n, cols, L, tbl()); }
