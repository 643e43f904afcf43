// posterior.h -- CTC forward-backward per label (include/ctcdecode_amd.h "Label posteriors"): for every label i of a hypothesis the
// state posterior g[t] = exp(a[t][s] + b[t][s] - lp(t, z[s]) - ll) of its state s = 2i + 1, reduced over the item's frames to the frame
// where it peaks, the expected number of frames the label occupies and the posterior-weighted mean of the model's probability of the
// label over them.  a is loglik.h's forward recurrence, ll its result, and b the same recurrence run on the reversed labels over the
// reversed frames; every operation is one float32 operation in a fixed order, so the outputs are defined bit for bit.
//
// Everything that defines the result is CTC_HD code here, compiled for both sides: e80, the g step, the accumulator update, and the
// slot and grid arithmetic of posterior.hip.  The kernel of posterior.hip walks a row twice by lattice_device.h's walk, forward with
// a kept in the row's scratch slot and then backward; posterior_row_host below runs the same cells sequentially, state by state in
// their own order (the host twin, tests/native/posterior_host.cpp).  lse3, the cell and the end rule are loglik.h's; the extended
// sequence, lp(t, c), the row validation and the entry prelude are align.h's.
#pragma once
#include "loglik.h"

namespace ctcpost {

using ctcalign::neg_inf;

constexpr long long kPostDefaultScratch = 2ll << 30;  // the budget of the scratch that keeps a

// ---- e80 and the g step ------------------------------------------------------------------------------------------------------------
// expf on [-80, 0]: an argument above 0 counts as 0 (the last-place excess rounding gives a + b - lp - ll), one below -80 gives 0.0f,
// so that e80 itself never leaves the normal range.  Branch-free around expf_nonpos, like lse3.
CTC_HD float e80(float x, const uint64_t *tbl) {
  const bool below = x < -80.0f;
  const float r = ctcmath::expf_nonpos(below || x > 0.0f ? 0.0f : x, tbl);
  return below ? 0.0f : r;
}
// g[t] of a state from a[t][s], b[t][s], lp(t, z[s]) and ll: 0 if a, b or their float sum is -inf
CTC_HD float g_step(float a, float b, float lp, float ll, const uint64_t *tbl) {
  const float ab = a + b;
  const bool none = !(a > neg_inf()) || !(b > neg_inf()) || !(ab > neg_inf());
  const float g = e80(none ? 0.0f : (ab - lp) - ll, tbl);
  return none ? 0.0f : g;
}

// ---- a label's accumulators, updated with g[t] in the order t = n - 1 .. 0 ----------------------------------------------------------
struct LabelAcc {
  float occ, num, best;  // the sums of g[t] and of g[t] * e80(lp(t, z[s])), from +0.0; the greatest g[t] so far
  int peak;              // the smallest t so far whose g[t] equals `best`
};
CTC_HD void acc_init(LabelAcc &c) {
  c.occ = 0.0f;
  c.num = 0.0f;
  c.best = 0.0f;
  c.peak = 0;
}
CTC_HD void acc_update(LabelAcc &c, int t, float g, float lp, const uint64_t *tbl) {
  c.occ = c.occ + g;
  c.num = c.num + g * e80(lp, tbl);
  if (g >= c.best) {  // (descending t: among equals the last one seen, the smallest)
    c.best = g;
    c.peak = t;
  }
}
CTC_HD float acc_confidence(const LabelAcc &c) { return c.occ == 0.0f ? 0.0f : c.num / c.occ; }

// ---- scratch slots and the grid ------------------------------------------------------------------------------------------------------
// A slot keeps a[t][s] of one workgroup's hypothesis in flight between its two walks -- frame t's S floats at t * S, for the longest
// extended sequence the shape allows -- or of four one-wave hypotheses (S <= 64: T * 64 floats each), whichever is larger.
CTC_HD size_t post_wave_floats(int T) { return (size_t)T * 64; }
CTC_HD size_t post_slot_bytes(int T, int L_stride) {
  const size_t row = (size_t)ctcalign::n_states(ctcalign::align_lmax(T, L_stride)), four = (size_t)ctcalign::kAlignWaves * 64;
  const size_t floats = (size_t)T * (row > four ? row : four);
  return (floats * 4 + 255) / 256 * 256;
}
// the grid = the rows, or the slots the budget pays for, at least one (the kernel of class 0 takes whole groups: at most the groups)
CTC_HD long long post_grid(long long rows, long long budget, size_t slot_bytes) {
  long long slots = (budget > 0 ? budget : kPostDefaultScratch) / (long long)(slot_bytes ? slot_bytes : 1);
  const long long g = rows < slots ? rows : slots;
  return g < 1 ? 1 : g;
}
// label i's state, and where state s' of the reversed labels lies among the row's own
CTC_HD int label_state(int i) { return 2 * i + 1; }
CTC_HD int mirrored_state(int S, int s) { return S - 1 - s; }

// ---- one hypothesis, sequentially (the host twin) ------------------------------------------------------------------------------------
// Row `tok` (L_stride words, `len` of them labels) of item b against the item's rows; slot: post_slot_bytes(T, L_stride) bytes of
// scratch.  peaks / occ / conf: L_stride words each, all written.  Returns 0, or ALIGN_BAD_ROW.
template <int DT, bool PROB>
inline int posterior_row_host(const void *probs, const int32_t *seq_lens, int b, int T, int V, int blank, const int32_t *tok, int len, int L_stride,
                              const uint64_t *tbl, float *slot, int32_t *peaks, float *occ, float *conf, float *loglik) {
  using namespace ctcalign;
  for (int i = 0; i < L_stride; ++i) {
    peaks[i] = 0;
    occ[i] = conf[i] = 0.0f;
  }
  int n;
  const int L = row_code_host(seq_lens, b, T, V, blank, tok, len, L_stride, &n), S = n_states(L);
  if (L < 0) {
    *loglik = no_row_score(L, len, n);
    return L == kRowInvalid ? ALIGN_BAD_ROW : 0;
  }
  const size_t row0 = (size_t)b * T;
  auto lp = [&](int t, int s) { return lp_at<DT, PROB>(probs, (row0 + (size_t)t) * V + (size_t)state_label(tok, s, blank)); };
  // the forward walk: a[t][s] at slot[t * S + s]
  for (int s = 0; s < S; ++s) slot[s] = s < 2 ? lp(0, s) : neg_inf();
  for (int t = 1; t < n; ++t) {
    const float *a = slot + (size_t)(t - 1) * S;
    float *na = slot + (size_t)t * S;
    for (int s = 0; s < S; ++s)
      na[s] = ctcloglik::cell_update(lp(t, s), a[s], s >= 1 ? a[s - 1] : neg_inf(), state_skips(tok, s) ? a[s - 2] : neg_inf(), tbl);
  }
  const float *a_end = slot + (size_t)(n - 1) * S;
  const float ll = ctcloglik::end_value(L, a_end[S - 1], L >= 1 ? a_end[S - 2] : neg_inf(), tbl);
  *loglik = ll;
  if (!(ll > neg_inf()) || L == 0) return 0;
  // the backward walk, frame n - 1 first; the labels' accumulators
  std::vector<float> bt((size_t)S), nb((size_t)S);
  std::vector<LabelAcc> acc((size_t)L);
  for (auto &c : acc) acc_init(c);
  for (int s = 0; s < S; ++s) bt[(size_t)s] = s >= S - 2 ? lp(n - 1, s) : neg_inf();
  for (int t = n - 1; t >= 0; --t) {
    if (t < n - 1) {
      for (int s = 0; s < S; ++s) {
        const bool skips = s + 2 <= S - 1 && state_skips(tok, s + 2);  // (odd s whose label differs from the next one)
        nb[(size_t)s] = ctcloglik::cell_update(lp(t, s), bt[(size_t)s], s + 1 <= S - 1 ? bt[(size_t)s + 1] : neg_inf(), skips ? bt[(size_t)s + 2] : neg_inf(), tbl);
      }
      bt.swap(nb);
    }
    for (int i = 0; i < L; ++i) {
      const int s = label_state(i);
      const float l = lp(t, s);
      acc_update(acc[(size_t)i], t, g_step(slot[(size_t)t * S + s], bt[(size_t)s], l, ll, tbl), l, tbl);
    }
  }
  for (int i = 0; i < L; ++i) {
    peaks[i] = acc[(size_t)i].peak;
    occ[i] = acc[(size_t)i].occ;
    conf[i] = acc_confidence(acc[(size_t)i]);
  }
  return 0;
}

// ---- what posterior.hip needs of the library's host file (ctcdecode_amd.hip), beyond align.h's hooks ---------------------------------
long long post_budget(const ctcd_decoder *d);  // ctcd_set_posterior_scratch (0: the default)
// the decoder's scratch for a, grown to `bytes`
int post_scratch(ctcd_decoder *d, size_t bytes, void **p);
void post_note_grid(ctcd_decoder *d, long long grid);  // ctcd_last_posterior_grid

}  // namespace ctcpost
