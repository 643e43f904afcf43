// loglik.h -- the CTC log-likelihood of a hypothesis (include/ctcdecode_amd.h "CTC log-likelihood"): log P(y | x), the sum over ALL
// alignments of y[0..L) through the item's n frames, by the forward recurrence over align.h's extended sequence z (S = 2L + 1 states)
//   a[t][s] = lp(t, z[s]) + lse3(a[t-1][s], a[t-1][s-1], a[t-1][s-2])
// -- align.h's Viterbi recurrence with the maximum replaced by a three-way float32 log-sum-exp whose expf / logf are glibc's, restated
// by exact_math.h, so the result is defined bit for bit.  No back-pointers, no scratch, no back-trace.
//
// Everything that defines the result is CTC_HD code here, compiled for both sides: lse3, the cell, the end rule, and the grid
// arithmetic of loglik.hip.  The kernel of loglik.hip spreads a frame's cells over the lanes of a wave or a workgroup, by the walk of
// lattice_device.h that it shares with align.hip; loglik_row_host below runs them sequentially (the host twin,
// tests/native/loglik_host.cpp).  The extended sequence, lp(t, c) for the three input modes, the row validation with its row codes and
// the entry prelude are align.h's.
#pragma once
#include "align.h"

namespace ctcloglik {

using ctcalign::neg_inf;

// ---- lse3 ------------------------------------------------------------------------------------------------------------------------
// logf((expf(v0 - m) + expf(v1 - m)) + expf(v2 - m)) + m with m = max(v0, v1, v2); -inf if m is -inf.  An absent argument is -inf.
// The first argument equal to m contributes expf(+0) = 1.0f exactly, so only the other two are evaluated (a and b, in the order they
// stand in the sum); expf_nonpos gives 0 for -inf and below -88, where glibc's value (< 2^-125) cannot change a float sum that holds
// a 1.0f.  Branch-free, so that the cells one lane holds stay independent instruction streams: with m = -inf the arithmetic runs on
// m = 0 (no NaN is ever formed) and the result is replaced at the end.  tbl: exact_math.h's 64 table words.
CTC_HD float max3(float v0, float v1, float v2) {
  const float m01 = v0 < v1 ? v1 : v0;
  return m01 < v2 ? v2 : m01;
}
CTC_HD float lse3(float v0, float v1, float v2, const uint64_t *tbl) {
  const float m = max3(v0, v1, v2);
  const bool none = !(m > neg_inf());
  const float ms = none ? 0.0f : m;
  const int imax = v0 == m ? 0 : (v1 == m ? 1 : 2);
  const float a = imax == 0 ? v1 : v0, b = imax == 2 ? v1 : v2;
  const float ea = ctcmath::expf_nonpos(a - ms, tbl), eb = ctcmath::expf_nonpos(b - ms, tbl);
  const float e0 = imax == 0 ? 1.0f : ea;
  const float e1 = imax == 0 ? ea : (imax == 1 ? 1.0f : eb);
  const float e2 = imax == 2 ? 1.0f : eb;
  const float sum = (e0 + e1) + e2;                        // in [1, 3]
  const float r = ctcmath::logf_normal(sum, tbl) + ms;     // (always evaluated: +0 + m for a lone predecessor, +0.0 for m = -0.0)
  return none ? neg_inf() : r;
}

// ---- the cell and the end rule ---------------------------------------------------------------------------------------------------
// stay = a[t-1][s]; p1 = a[t-1][s-1] and p2 = a[t-1][s-2], or -inf where that predecessor does not exist or is not allowed
CTC_HD float cell_update(float lp, float stay, float p1, float p2, const uint64_t *tbl) { return lp + lse3(stay, p1, p2, tbl); }
// a_last = a[n-1][S-1], a_before = a[n-1][S-2] (looked at only if L >= 1)
CTC_HD float end_value(int L, float a_last, float a_before, const uint64_t *tbl) { return lse3(a_last, L >= 1 ? a_before : neg_inf(), neg_inf(), tbl); }

// ---- the grid --------------------------------------------------------------------------------------------------------------------
// The rows are classed as align.h's: a group of four consecutive rows that all fit a wave runs side by side (class 0, unit = the
// group); any other row runs on the whole workgroup with 1, 4 or 16 states per lane (class = align_npl(S), unit = the row).  A
// workgroup takes the units blockIdx.x, + gridDim.x, ...; no scratch binds the grid, so it is min(units, cap): the caller's cap
// (ctcd_set_loglik_grid), or by default the workgroups the device holds at once -- its compute units times the workgroups of four
// waves (one per SIMD) the class's registers allow on one, the least over its instantiations: 512 / VGPRs, and 7 at most with more
// than 96 SGPRs (DESIGN.md 2i has the register counts).  A grid beyond that would only queue; one below it leaves SIMDs idle.
CTC_HD long long loglik_units(long long rows, int cls) { return cls == 0 ? ctcalign::align_groups(rows) : rows; }
CTC_HD int loglik_occupancy(int cls) { return cls == 16 ? 2 : (cls == 4 ? 4 : (cls == 1 ? 7 : 6)); }
CTC_HD long long loglik_grid(long long units, long long cap, int cus, int cls) {
  long long g = cap > 0 ? cap : (long long)(cus > 0 ? cus : 1) * loglik_occupancy(cls);
  if (g > units) g = units;
  return g < 1 ? 1 : g;
}

// ---- one hypothesis, sequentially (the host twin) ----------------------------------------------------------------------------------
// Row `tok` (`len` labels of at most L_stride) of item b against the item's rows.  Returns 0, or ALIGN_BAD_ROW (*out = 0).
template <int DT, bool PROB>
inline int loglik_row_host(const void *probs, const int32_t *seq_lens, int b, int T, int V, int blank, const int32_t *tok, int len, int L_stride,
                           const uint64_t *tbl, float *out) {
  using namespace ctcalign;
  int n;
  const int L = row_code_host(seq_lens, b, T, V, blank, tok, len, L_stride, &n), S = n_states(L);
  if (L < 0) {
    *out = no_row_score(L, len, n);
    return L == kRowInvalid ? ALIGN_BAD_ROW : 0;
  }
  const size_t row0 = (size_t)b * T;
  std::vector<float> a((size_t)S), na((size_t)S);
  for (int s = 0; s < S; ++s) a[(size_t)s] = s < 2 ? lp_at<DT, PROB>(probs, row0 * V + (size_t)state_label(tok, s, blank)) : neg_inf();
  for (int t = 1; t < n; ++t) {
    for (int s = 0; s < S; ++s) {
      const float lp = lp_at<DT, PROB>(probs, (row0 + (size_t)t) * V + (size_t)state_label(tok, s, blank));
      na[(size_t)s] = cell_update(lp, a[(size_t)s], s >= 1 ? a[(size_t)s - 1] : neg_inf(), state_skips(tok, s) ? a[(size_t)s - 2] : neg_inf(), tbl);
    }
    a.swap(na);
  }
  *out = end_value(L, a[(size_t)S - 1], L >= 1 ? a[(size_t)S - 2] : neg_inf(), tbl);
  return 0;
}

// ---- what loglik.hip needs of the library's host file (ctcdecode_amd.hip), beyond align.h's hooks ----------------------------------
struct LoglikDecoderInfo {
  long long cap;  // ctcd_set_loglik_grid (0: the default)
  int cus;        // the device's compute units
};

}  // namespace ctcloglik

namespace ctcloglik {
int loglik_decoder_info(const ctcd_decoder *d, LoglikDecoderInfo *out);
void loglik_note_grid(ctcd_decoder *d, long long grid);  // ctcd_last_loglik_grid
}  // namespace ctcloglik
