// keyword.h -- keyword search (include/ctcdecode_amd.h "Keyword search"): for every keyword k[0..L) and every item, the window of the
// item's frames in which the keyword's best path scores highest against the best unconstrained path over the same frames -- the
// keyword-filler model.  A Viterbi pass over the keyword's S = 2L - 1 states (z[2i] = k[i], z[2i+1] = blank) with a free start and a
// free end, on rows taken relative to the frame's greatest value: r(t, c) = lp(t, c) - m(t).  A cell is a pair (value, start frame):
// the start travels with the path, so there is no back-pointer scratch and no back-trace.  One subtraction, one addition and exact
// maxima per cell: the result is defined bit for bit.
//
// Everything that defines the result is CTC_HD code here, compiled for both sides: the relative value, the two cell updates with
// their tie rule, the walk over the end state that picks the window, the validation, and the shape arithmetic of the launch (lane
// group, staging route).  The kernel of keyword.hip puts a keyword's labels on the lanes of a lane group; keyword_item_host below
// runs the same routines sequentially (the host twin, tests/native/keyword_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "greedy.h"

namespace ctckw {

using ctcalign::neg_inf;
using ctcgreedy::FrameRec;

enum : int { KW_BAD = ctcalign::ALIGN_BAD_ROW };  // the status word of an invalid keyword

constexpr int kKwMaxLabels = 64;    // a keyword's labels lie on the lanes of one wave
constexpr int kKwThreads = 256;     // the kernel's workgroup: four waves, all on the same item's frames
constexpr int kKwChunk = 32;        // F: the frames staged (or prefetched) at a time
constexpr int kKwStagedMaxV = 128;  // the widest row whose chunks are staged in LDS (two buffers of F * V floats: 32 KiB at most)

// ---- the rows ----------------------------------------------------------------------------------------------------------------------
// r(t, c): -inf where lp is, else one float32 subtraction of the frame's greatest lp (greedy.h FrameRec::lp)
CTC_HD float rel(float lp, float m) { return lp == neg_inf() ? neg_inf() : lp - m; }

// ---- the cell ----------------------------------------------------------------------------------------------------------------------
struct Pair {
  float v;
  int32_t s;  // the frame at which the path entered state 0
};
CTC_HD Pair no_path() {
  Pair p;
  p.v = neg_inf();
  p.s = -1;
  return p;
}
CTC_HD int kw_states(int L) { return 2 * L - 1; }
// A label state 2i.  i >= 1: stay, before the blank state in front of it (p1), before the label state in front of that (p2, where the
// two labels differ: has2).  i == 0: stay, before the entry (0.0f, t) -- the filler path, whose relative score is 0.  Strict `>`.
CTC_HD Pair label_cell(float r, Pair stay, Pair p1, Pair p2, bool has2, bool first, int t) {
  Pair best = stay;
  if (!first && p1.v > best.v) best = p1;
  if (!first && has2 && p2.v > best.v) best = p2;
  if (first && 0.0f > best.v) {
    best.v = 0.0f;
    best.s = t;
  }
  best.v = r + best.v;
  return best;
}
// A blank state 2i + 1: stay, before the label state in front of it
CTC_HD Pair blank_cell(float r, Pair stay, Pair p1) {
  Pair best = stay;
  if (p1.v > best.v) best = p1;
  best.v = r + best.v;
  return best;
}

// ---- the result --------------------------------------------------------------------------------------------------------------------
// the walk over d[t][S - 1], t = 0 .. n - 1: the latest frame that attains the maximum wins (`>=`)
struct Hit {
  float v;
  int32_t s, e;
};
CTC_HD Hit no_hit() {
  Hit h;
  h.v = neg_inf();
  h.s = h.e = -1;
  return h;
}
CTC_HD void hit_step(Hit &h, Pair d, int t) {
  if (d.v >= h.v) {
    h.v = d.v;
    h.s = d.s;
    h.e = t;
  }
}
// no window at all: start = end = -1
CTC_HD Hit hit_final(Hit h) {
  if (!(h.v > neg_inf())) h.s = h.e = -1;
  return h;
}
// an invalid keyword: score 0, start = end = -1
CTC_HD Hit bad_hit() {
  Hit h;
  h.v = 0.0f;
  h.s = h.e = -1;
  return h;
}

// ---- validation and the launch's shapes ----------------------------------------------------------------------------------------------
CTC_HD bool kw_len_ok(int L, int L_stride) { return L >= 1 && L <= L_stride; }
// the lanes a keyword occupies: the least of 8, 16, 32, 64 that holds L_stride labels (log2)
CTC_HD int lane_group_log2(int L_stride) { return L_stride <= 8 ? 3 : (L_stride <= 16 ? 4 : (L_stride <= 32 ? 5 : 6)); }
CTC_HD int kw_per_workgroup(int lg) { return kKwThreads >> lg; }
CTC_HD bool kw_staged(int V) { return V <= kKwStagedMaxV; }
CTC_HD size_t kw_lds_bytes(int V) { return kw_staged(V) ? (size_t)2 * kKwChunk * (size_t)V * sizeof(float) : 0; }
// what ctcd_last_keyword_kernel reports: the instantiation (DT, PROB, STAGED) and the lane-group width
CTC_HD int kw_kernel_code(int dt, bool prob, bool staged, int lg) { return ((dt | (prob ? 4 : 0) | (staged ? 8 : 0)) << 8) | (1 << lg); }

// ---- one keyword against one item, sequentially (the host twin) --------------------------------------------------------------------
// rec: the item's frame records (greedy.h frame_recs_host on the rows read here); kw: L_stride words, `len` of them labels.
// tr_v / tr_s: T words each or NULL, all written.  Returns 0, or KW_BAD.
template <int DT, bool PROB>
inline int keyword_item_host(const void *probs, int b, int T, int V, int n, int blank, const FrameRec *rec, const int32_t *kw, int len, int L_stride, float *score,
                             int32_t *start, int32_t *end, float *tr_v, int32_t *tr_s) {
  for (int t = 0; tr_v && t < T; ++t) {
    tr_v[t] = 0.0f;
    tr_s[t] = 0;
  }
  bool ok = kw_len_ok(len, L_stride);
  for (int i = 0; ok && i < len; ++i) ok = ctcalign::label_ok(kw[i], V, blank);
  Hit h = bad_hit();
  if (ok) {
    const int S = kw_states(len);
    std::vector<Pair> d((size_t)S, no_path()), nd((size_t)S);
    h = no_hit();
    for (int t = 0; t < n; ++t) {
      const size_t row0 = ((size_t)b * T + (size_t)t) * V;
      for (int s = 0; s < S; ++s) {
        const int c = (s & 1) ? blank : kw[s >> 1];
        const float r = rel(ctcalign::lp_at<DT, PROB>(probs, row0 + (size_t)c), rec[t].lp);
        if (s & 1) nd[(size_t)s] = blank_cell(r, d[(size_t)s], d[(size_t)s - 1]);
        else nd[(size_t)s] = label_cell(r, d[(size_t)s], s ? d[(size_t)s - 1] : no_path(), s ? d[(size_t)s - 2] : no_path(), s && kw[s >> 1] != kw[(s >> 1) - 1], s == 0, t);
      }
      d.swap(nd);
      hit_step(h, d[(size_t)S - 1], t);
      if (tr_v) {
        tr_v[t] = d[(size_t)S - 1].v;
        tr_s[t] = d[(size_t)S - 1].s;
      }
    }
    h = hit_final(h);
  }
  *score = h.v;
  *start = h.s;
  *end = h.e;
  return ok ? 0 : KW_BAD;
}

}  // namespace ctckw

struct ctcd_decoder;
namespace ctckw {
// what keyword.hip needs of the library's host file (ctcdecode_amd.hip) beyond align.h's and greedy.h's hooks
void keyword_note_kernel(ctcd_decoder *d, int code);  // ctcd_last_keyword_kernel
}  // namespace ctckw
