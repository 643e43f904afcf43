// loglik_grad.h -- the gradient of the CTC log-likelihood (include/ctcdecode_amd.h "Log-likelihood gradient"): for every row of an
// item the state posteriors g[t][s] of posterior.h, for the blank states as well as the labels', summed per frame over the states
// that share a label, weighted with the row's weight and accumulated over the item's rows into one [T][V] slab.  a, b, ll, e80 and the
// g step are posterior.h's; what is new is the ORDER of the float32 sums, which is what makes the result a function of the inputs alone.
//
// Everything that defines the result is CTC_HD code here, compiled for both sides: the weighted value, the chain of a label's
// positions and the tree of the blank's states.  The kernel of loglik_grad.hip computes the same sums spread over lanes and waves.
#pragma once
#include "posterior.h"

namespace ctcgrad {

using ctcalign::neg_inf;

// w * g[t][s], two float32 operations.  The + 0.0f turns a -0.0 (w < 0, g == 0) into +0.0, so that no sum below ever sees one: with
// that, x + (+0.0) == x for every x that occurs, and padding a sum with +0.0 or leaving a term of weight 0 out changes no bit.
CTC_HD float weighted(float w, float g) { return w * g + 0.0f; }

// A label's total of one frame: the weighted values of its positions i_0 < i_1 < .. of the row, x[i_0] + x[i_1] + .., left to right.
CTC_HD float chain_sum(const float *x, const int *pos, int count) {
  float s = x[pos[0]];
  for (int i = 1; i < count; ++i) s = s + x[pos[i]];
  return s;
}

// The blank's total of one frame: its states counted from the row's end, e = (S - 1 - s) / 2 = 0 .. L, summed pairwise level by level
// -- x[2m] + x[2m + 1], a missing right element counts as +0.0 -- until one value is left.  x is overwritten.
CTC_HD float blank_tree(float *x, int count) {
  for (; count > 1; count = (count + 1) / 2)
    for (int m = 0; 2 * m < count; ++m) x[m] = x[2 * m] + (2 * m + 1 < count ? x[2 * m + 1] : 0.0f);
  return x[0];
}
// the same tree over the 1 / 2 / 8 blank states a lane holds (NPL states per lane, the even ones; v: the lane's weighted values)
template <int NPL> CTC_HD float lane_blank_tree(const float (&v)[NPL], bool first_is_even) {
  if (NPL == 1) return first_is_even ? v[0] : 0.0f;
  if (NPL == 4) return v[0] + v[NPL >= 4 ? 2 : 0];
  float q[NPL / 2 > 0 ? NPL / 2 : 1];
  for (int i = 0; i < NPL / 2; ++i) q[i] = v[2 * i];
  return blank_tree(q, NPL / 2);
}

}  // namespace ctcgrad
