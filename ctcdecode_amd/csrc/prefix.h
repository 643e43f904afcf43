// prefix.h -- CTC prefix scores (include/ctcdecode_amd.h "CTC prefix scores"): what a label-synchronous decoder asks at every step.
// A prefix g of L labels is kept as the column of its last two lattice states per frame -- r_n[t] = a[t][S-2], r_b[t] = a[t][S-1]
// of loglik.h's recurrence for y = g, the pair a band of a long row hands to the next one -- and three operations work on it:
//   init     the empty prefix: the blank column's running sum
//   advance  g -> g.c: the lattice cell of the two new states, one lse3 each per frame, from the parent's column
//   scores   psi(g.c) for many candidates c at once: log sum_t exp(lp(t, c) + phi[t-1]), phi the parent's column folded per frame,
//            by one sequential pass over a pair (m, s) -- one expf per (prefix, candidate, frame), one logf per (prefix, candidate)
// and the end score eos(g) = log_likelihood(g), bit for bit.
//
// Everything that defines the results is CTC_HD code here, compiled for both sides: the (m, s) step and its end, phi, the advance
// cell, the validity rules and the launch arithmetic of prefix.hip.  The kernels of prefix.hip spread candidates and prefixes over
// lanes; the *_host routines below run them sequentially (the host twin, tests/native/prefix_host.cpp).  lse3 is loglik.h's, lp(t, c)
// for the three input modes align.h's.
#pragma once
#include "loglik.h"

namespace ctcprefix {

using ctcalign::neg_inf;
using ctcloglik::lse3;

// ---- validity ----------------------------------------------------------------------------------------------------------------------
// A slot: lens < 0 is unused; a prefix of L >= 1 labels whose `last` is no label of the vocabulary is invalid (the item's status word
// is raised); `last` of the empty prefix is not looked at.  -> L, or one of the codes.
enum : int { kSlotUnused = -1, kSlotBad = -2 };
CTC_HD int slot_code(int len, int last, int V, int blank) { return len < 0 ? kSlotUnused : (len >= 1 && !ctcalign::label_ok(last, V, blank) ? kSlotBad : len); }
// A candidate: -1 and the blank score -inf; anything else outside [0, V) scores -inf and raises the item's status word.
enum : int { kCandNone = 0, kCandBad = 1, kCandOk = 2 };
CTC_HD int cand_code(int c, int V, int blank) { return (c == -1 || c == blank) ? kCandNone : ((unsigned)c >= (unsigned)V ? kCandBad : kCandOk); }

// ---- the column ----------------------------------------------------------------------------------------------------------------------
struct Pair {
  float n, b;  // r_n[t], r_b[t]: cols[..., t, 0] and cols[..., t, 1]
};
// init: frame 0, and frame t from frame t - 1
CTC_HD Pair init_first(float lp_blank) { return Pair{neg_inf(), lp_blank}; }
CTC_HD Pair init_cell(float lp_blank, Pair prev, const uint64_t *tbl) { return Pair{neg_inf(), lp_blank + lse3(prev.b, neg_inf(), neg_inf(), tbl)}; }
// advance by c: frame 0, and frame t from the child's and the parent's pairs of frame t - 1; differs: the parent is empty or c != its last
CTC_HD Pair advance_first(float lp_c, bool parent_empty) { return Pair{parent_empty ? lp_c : neg_inf(), neg_inf()}; }
CTC_HD Pair advance_cell(float lp_c, float lp_blank, Pair child, Pair parent, bool differs, const uint64_t *tbl) {
  Pair r;
  r.n = lp_c + lse3(child.n, parent.b, differs ? parent.n : neg_inf(), tbl);
  r.b = lp_blank + lse3(child.b, child.n, neg_inf(), tbl);
  return r;
}
// eos of a prefix of L labels from its pair at frame n - 1 (n >= 1), and without frames
CTC_HD float eos_value(int L, Pair p, const uint64_t *tbl) { return ctcloglik::end_value(L, p.b, p.n, tbl); }
CTC_HD float eos_no_frames(int L) { return L == 0 ? 0.0f : neg_inf(); }

// ---- the prefix score ------------------------------------------------------------------------------------------------------------------
// phi[t] for a candidate that differs from the prefix's last label (one that equals it takes r_b[t] itself)
CTC_HD float phi_all(Pair p, const uint64_t *tbl) { return lse3(p.b, p.n, neg_inf(), tbl); }
// what stands for phi[-1]: v[0] = lp(0, c) + (-0.0f) is lp(0, c) with every bit kept (-0.0 is float addition's identity), or -inf
CTC_HD float phi_before_first(int L) { return L == 0 ? -0.0f : neg_inf(); }
// the running sum: exp(m) * s = the sum of the exp(v) so far; a term of -inf is skipped.  s >= 1 once a term was taken, so an expf
// below 2^-126 (expf_nonpos gives 0 there) cannot change it.  Branch-free: with v = -inf the arithmetic runs on d = 0 and is dropped.
struct Sum {
  float m, s;
};
CTC_HD Sum sum_none() { return Sum{neg_inf(), 0.0f}; }
CTC_HD void sum_step(Sum &a, float v, const uint64_t *tbl) {
  const bool take = v > neg_inf(), up = v > a.m;
  const float d = !take ? 0.0f : (up ? a.m - v : v - a.m);  // <= 0; -inf for the first term
  const float e = ctcmath::expf_nonpos(d, tbl);
  const float prod = a.s * e;
  const float s = up ? prod + 1.0f : a.s + e;
  a.s = take ? s : a.s;
  a.m = take && up ? v : a.m;
}
CTC_HD float sum_final(Sum a, const uint64_t *tbl) {
  const float r = ctcmath::logf_normal(a.s >= 1.0f ? a.s : 1.0f, tbl) + a.m;  // (s in [1, n]: logf_normal holds for every normal float)
  return a.m > neg_inf() ? r : neg_inf();
}

// ---- the launches of prefix.hip ----------------------------------------------------------------------------------------------------
constexpr int kPxThreads = 256;      // the scores kernel's workgroup: four waves
constexpr int kPxChunk = 32;         // F: frames of a chunk (one barrier pair per chunk)
constexpr int kPxSlots = 8;          // H: prefixes one lane scores its candidate against (all labels as candidates)
constexpr int kPxMaxWgSlots = 64;    // prefixes of one workgroup at most: eight lane groups of H
constexpr int kPxAhead = 8;          // gathered rows: frames a lane loads ahead
constexpr int kPxStagedMaxV = 128;   // rows of at most this many labels are staged in LDS (keyword.h kKwStagedMaxV)
constexpr int kPxAdvThreads = 64;    // the advance kernel's workgroup: one wave, one new prefix per lane
constexpr int kPxAdvFrames = 16;     // ... and the frames of its LDS tile
CTC_HD bool px_staged(int V) { return V <= kPxStagedMaxV; }
CTC_HD size_t px_lds_bytes(int V) { return px_staged(V) ? (size_t)kPxChunk * (size_t)V * sizeof(float) : 0; }
// a workgroup's lanes form 256 / W groups of W = 32 .. 256 lanes, one candidate per lane: the narrowest that holds the C candidates
CTC_HD int px_group_log2(int C) { return C <= 32 ? 5 : (C <= 64 ? 6 : (C <= 128 ? 7 : 8)); }
// prefixes per lane group: one with listed candidates (every prefix has a list of its own); with all labels as candidates as many
// as spread R over the groups, H at most
CTC_HD int px_group_slots(bool listed, int R, int lg) {
  if (listed) return 1;
  const int G = kPxThreads >> lg, hs = (R + G - 1) / G;
  return hs < 1 ? 1 : (hs > kPxSlots ? kPxSlots : hs);
}
// what ctcd_last_prefix_kernel reports: the instantiation and the route
enum : int { kPxKindScores = 0, kPxKindAdvance = 1, kPxKindInit = 2 };
CTC_HD int px_kernel_code(int kind, int dt, bool prob, bool staged, bool listed, int lg, int hs) {
  return dt | (prob ? 4 : 0) | (staged ? 8 : 0) | (listed ? 16 : 0) | (kind << 5) | (lg << 8) | (hs << 12);
}

// ---- sequentially (the host twin) ----------------------------------------------------------------------------------------------------
// cols: the T pairs of one slot.  n: the item's frames.
template <int DT, bool PROB>
inline void init_host(const void *probs, size_t row0, int n, int V, int blank, const uint64_t *tbl, float *cols) {
  Pair p{};
  for (int t = 0; t < n; ++t) {
    const float lb = ctcalign::lp_at<DT, PROB>(probs, (row0 + (size_t)t) * V + (size_t)blank);
    p = t == 0 ? init_first(lb) : init_cell(lb, p, tbl);
    cols[2 * t] = p.n, cols[2 * t + 1] = p.b;
  }
}
// the parent (pcols, L labels, the last one `last`) advanced by the valid label c into ccols
template <int DT, bool PROB>
inline void advance_host(const void *probs, size_t row0, int n, int V, int blank, const float *pcols, int L, int last, int c, const uint64_t *tbl, float *ccols) {
  Pair ch{}, pa{};
  for (int t = 0; t < n; ++t) {
    const float lc = ctcalign::lp_at<DT, PROB>(probs, (row0 + (size_t)t) * V + (size_t)c), lb = ctcalign::lp_at<DT, PROB>(probs, (row0 + (size_t)t) * V + (size_t)blank);
    ch = t == 0 ? advance_first(lc, L == 0) : advance_cell(lc, lb, ch, pa, L == 0 || c != last, tbl);
    pa = Pair{pcols[2 * t], pcols[2 * t + 1]};
    ccols[2 * t] = ch.n, ccols[2 * t + 1] = ch.b;
  }
}
// psi(g.c) for the valid candidate c
template <int DT, bool PROB>
inline float score_host(const void *probs, size_t row0, int n, int V, const float *cols, int L, int last, int c, const uint64_t *tbl) {
  Sum a = sum_none();
  for (int t = 0; t < n; ++t) {
    float prev = phi_before_first(L);
    if (t > 0) {
      const Pair p{cols[2 * (t - 1)], cols[2 * (t - 1) + 1]};
      prev = (L >= 1 && c == last) ? p.b : phi_all(p, tbl);
    }
    sum_step(a, ctcalign::lp_at<DT, PROB>(probs, (row0 + (size_t)t) * V + (size_t)c) + prev, tbl);
  }
  return sum_final(a, tbl);
}
inline float eos_host(int n, const float *cols, int L, const uint64_t *tbl) {
  return n == 0 ? eos_no_frames(L) : eos_value(L, Pair{cols[2 * (n - 1)], cols[2 * (n - 1) + 1]}, tbl);
}

// ---- what prefix.hip needs of the library's host file (ctcdecode_amd.hip), beyond align.h's hooks ----------------------------------
void prefix_note_kernel(ctcd_decoder *d, int code);  // ctcd_last_prefix_kernel

}  // namespace ctcprefix
