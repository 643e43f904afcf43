// greedy.h -- greedy (best-path) CTC decoding (include/ctcdecode_amd.h "Greedy decode"): every frame's label is the index of its
// greatest input value, repeats collapse, blanks drop; the score is the float32 sum, in frame order, of the winners' log-probabilities
// -- the score of the path `align` finds for the row this decode returns.  Nothing is searched, so the result is defined bit for bit
// by three small rules.
//
// Everything that defines the result is CTC_HD code here, compiled for both sides: the argmax step and the rule that combines two
// partial winners, a winner's log-probability in the three input modes, the emit and run-end rules, the run and score bookkeeping,
// and the scratch arithmetic.  The kernels of greedy.hip spread a frame's labels over lanes and an item's frames over a workgroup;
// greedy_item_host below runs the same routines sequentially (the host twin, tests/native/greedy_host.cpp).  Live streams ("live
// streams" below; greedy_stream.hip, greedy_stream_item_host, tests/native/greedy_stream_host.cpp) add the record a stream keeps
// between chunk calls and the rules of what a call closes and leaves open.
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdint.h>

#include "align.h"
#include "exact_math.h"

namespace ctcgreedy {

using ctcalign::neg_inf;

// ---- the frame label ---------------------------------------------------------------------------------------------------------------
// A partial winner: the greatest value met so far and its index.  "None yet" has the value -inf and an index beyond every label, so
// that a frame of -inf alone ends at label 0 (winner_label) as the walk from c = 0 with a strict `>` does.
constexpr int kNoLabel = 0x7fffffff;
struct Winner {
  float v;
  int c;
};
CTC_HD Winner no_winner() {
  Winner w;
  w.v = neg_inf();
  w.c = kNoLabel;
  return w;
}
// the walk's step, for indices that come in increasing order: an ordered, strict `>` (equal values keep the smaller index; NaN never wins)
CTC_HD void argmax_step(Winner &w, float v, int c) {
  if (v > w.v) {
    w.v = v;
    w.c = c;
  }
}
// two partial winners of disjoint index sets: the greater value, else the smaller index (-0.0 and +0.0 are equal)
CTC_HD Winner argmax_combine(Winner a, Winner b) {
  const bool take_b = b.v > a.v || (!(a.v > b.v) && b.c < a.c);
  return take_b ? b : a;
}
// the frame's label; an index no label has (nothing but -inf, or NaN, was met) is label 0: always inside [0, V)
CTC_HD int winner_label(Winner w, int V) { return (unsigned)w.c < (unsigned)V ? w.c : 0; }

// ---- the winner's log-probability --------------------------------------------------------------------------------------------------
enum : int { kModeProb = 0, kModeLog = 1, kModeLogits = 2 };  // include/ctcdecode_amd.h log_input
// log_input == 2: the value ctcd_log_softmax writes for an element x of a frame with maximum m (a zero maximum taken as +0) and
// logsum = logf(sum of exponentials)
CTC_HD float lsm_value(float x, float m, float logsum) { return m > neg_inf() ? (x - m) - logsum : neg_inf(); }
CTC_HD float lsm_max(float greatest) { return greatest + 0.0f; }
// log_input 0 / 1 need the winner's value alone
template <int MODE> CTC_HD float winner_lp(float x) { return MODE == kModeProb ? ctcalign::prob_to_lp(x) : x; }

// ---- emission, runs and the score --------------------------------------------------------------------------------------------------
// frame t emits its label c: not the blank, and the first frame or another label than the frame before it (prev)
CTC_HD bool emits(int c, int prev, bool first, int blank) { return c != blank && (first || c != prev); }
// frame t is the last of a run of a label: not the blank, and the item's last frame or another label behind it (next)
CTC_HD bool run_ends(int c, int next, bool last, int blank) { return c != blank && (last || next != c); }
// the greatest lp of a run, exact; among equal values (-0.0, +0.0) the earliest frame's -- forward (the later frame needs a strict
// `>`) and backward (the earlier frame takes a tie)
CTC_HD float run_max_fwd(float acc, float later) { return later > acc ? later : acc; }
CTC_HD float run_max_back(float acc, float earlier) { return earlier >= acc ? earlier : acc; }
// the score: lp of frame 0, then one float32 addition per frame, in frame order
CTC_HD float score_step(float score, float lp, bool first) { return first ? lp : score + lp; }

// ---- live streams ------------------------------------------------------------------------------------------------------------------
// include/ctcdecode_amd.h "Greedy decode of live streams": what a stream carries from one chunk call to the next, so that its calls
// return, piece by piece, the decode of all frames it was ever fed.  One record of 32 bytes in device memory per stream; the kernel
// reads it at the start of a call and one thread writes it back at the end.
struct StreamRec {
  int32_t frames;    // frames fed so far (N)
  int32_t prev;      // c*(N - 1); meaningless while frames == 0
  int32_t emitted;   // labels emitted so far
  int32_t closed;    // runs closed so far (= emitted, less the open one)
  float score;       // the score of the frames so far; 0.0f while frames == 0
  float open_max;    // the greatest lp so far of the open run; 0.0f without one
  int32_t flags;     // kRecOpen | kRecEnded
  int32_t first;     // F0: added to every frame number reported
};
static_assert(sizeof(StreamRec) == 32, "the record of a greedy stream is 32 bytes");
enum : int { kRecOpen = 1, kRecEnded = 2 };
constexpr long long kStreamMaxFrame = 0x7fffffffLL;  // F0 + the frames fed stays at or below it
CTC_HD StreamRec stream_rec_init(int first_frame) {
  StreamRec r;
  r.frames = r.prev = r.emitted = r.closed = r.flags = 0;
  r.score = r.open_max = 0.0f;
  r.first = first_frame;
  return r;
}
CTC_HD bool rec_open(const StreamRec &r) { return (r.flags & kRecOpen) != 0; }
// the label in front of the chunk's frame 0 (emits does not look at it for the stream's first frame)
CTC_HD int rec_prev(const StreamRec &r, int blank) { return r.frames > 0 ? r.prev : blank; }
// chunk frame t is the first frame the stream ever had
CTC_HD bool stream_first(const StreamRec &r, int t) { return r.frames == 0 && t == 0; }
// the number reported for chunk frame t
CTC_HD int stream_frame_no(const StreamRec &r, int t) { return r.first + r.frames + t; }
// the run that came in open ends at the frame before this chunk: the chunk of n frames begins with another label (label0), or is empty and
// ends the stream.  It is closed entry 0 of the call: end stream_frame_no(r, -1), maximum r.open_max.
CTC_HD bool carried_closes(const StreamRec &r, int n, int label0, bool eos) { return rec_open(r) && (n > 0 ? label0 != r.prev : eos); }
// chunk frame t of n is known to be the last of its run: its successor is in the chunk, or the stream ends with the chunk
CTC_HD bool stream_run_ends(int c, int next, int t, int n, bool eos, int blank) { return (t + 1 < n || eos) && run_ends(c, next, t == n - 1, blank); }
// ... or its run stays open: the chunk's last frame of a stream that goes on
CTC_HD bool stream_run_open(int c, int t, int n, bool eos, int blank) { return c != blank && t == n - 1 && !eos; }
// the record behind a chunk of n frames whose last label is last_label (n > 0), in which `emitted` labels were emitted and `closed` runs
// closed; score: the score including the chunk; open_max: the maximum of the run stream_run_open found (n > 0)
CTC_HD StreamRec stream_rec_after(const StreamRec &r, int n, int last_label, int emitted, int closed, float score, float open_max, bool eos, int blank) {
  StreamRec a = r;
  a.frames = r.frames + n;
  a.emitted = r.emitted + emitted;
  a.closed = r.closed + closed;
  a.score = score;
  if (n > 0) a.prev = last_label;
  const bool open = !eos && (n > 0 ? last_label != blank : rec_open(r));
  a.open_max = open ? (n > 0 ? open_max : r.open_max) : 0.0f;
  a.flags = (open ? kRecOpen : 0) | (eos ? kRecEnded : 0);
  return a;
}

// ---- scratch -----------------------------------------------------------------------------------------------------------------------
// what the argmax pass leaves the collapse pass: 8 bytes per frame, frame t of item b at b * T + t
struct FrameRec {
  int32_t c;  // c*(t)
  float lp;   // lp(t, c*(t))
};
CTC_HD size_t greedy_scratch_bytes(long long B, long long T) { return ((size_t)B * (size_t)T * sizeof(FrameRec) + 255) / 256 * 256; }

// ---- the argmax pass's shapes ------------------------------------------------------------------------------------------------------
// Rows of up to 64 labels share a wave: G lanes per frame, the least power of two that holds the row.  Longer rows take a wave each,
// or -- beyond kWgMinV labels, when their rows are whole vectors (vec_rows) -- a workgroup of four.
constexpr int kWgMinV = 256;
constexpr int kLogitsMaxV = 16384;  // the longest row the logit kernels hold in registers (1024 * F4, F4 <= 16)
CTC_HD int lanes_per_frame(int V) {
  int g = 1;
  while (g < 64 && g < V) g <<= 1;
  return g;
}
// elements of one vector load: 16 bytes, except that half logits come four at a time (the thread-to-label mapping that fixes the
// log-softmax's summation order is the float32 one)
CTC_HD int vec_elems(int dtype, int mode) { return dtype == ctcskip::kSkipF32 || mode == kModeLogits ? 4 : 8; }
CTC_HD bool vec_rows(uintptr_t base, int V, int dtype, int mode) {
  const int e = vec_elems(dtype, mode);
  return V > kWgMinV && V % e == 0 && base % ((uintptr_t)e * ctcskip::elem_bytes(dtype)) == 0 && (mode != kModeLogits || V <= kLogitsMaxV);
}
CTC_HD int logits_f4(int V) { return V <= 1024 ? 1 : (V <= 2048 ? 2 : (V <= 4096 ? 4 : (V <= 10240 ? 10 : 16))); }

// ---- one item, sequentially (the host twin) ------------------------------------------------------------------------------------------
// The sum of exponentials of a frame in the order ctcd_log_softmax defines: 64 chains, chain l over the terms j = l, l + 64, ... in
// increasing j, then a butterfly over the chains (l ^ 1, ^ 2, ... ^ 32).
template <int DT> inline float lsm_sum_host(const void *rows, size_t row0, int V, float m, const uint64_t *tbl) {
  float p[64], q[64];
  for (int l = 0; l < 64; ++l) p[l] = 0.0f;
  for (int j = 0; j < V; ++j) p[j & 63] += ctcmath::expf_nonpos(ctcskip::widen_at<DT>(rows, row0 + (size_t)j) - m, tbl);
  for (int off = 1; off < 64; off <<= 1) {
    for (int l = 0; l < 64; ++l) q[l] = p[l] + p[l ^ off];
    for (int l = 0; l < 64; ++l) p[l] = q[l];
  }
  return p[0];
}

// Item b.  rec: the item's T frame records (scratch); tok / st / en / ls: T words each (en, ls may be NULL), all written; tbl:
// exact_math.h's 64 table words (MODE 2).
// the argmax pass: the records of item b's first n frames
template <int DT, int MODE> inline void frame_recs_host(const void *probs, int b, int T, int V, int n, const uint64_t *tbl, FrameRec *rec) {
  for (int t = 0; t < n; ++t) {
    const size_t row0 = ((size_t)b * T + (size_t)t) * V;
    Winner w = no_winner();
    for (int c = 0; c < V; ++c) argmax_step(w, ctcskip::widen_at<DT>(probs, row0 + (size_t)c), c);
    rec[t].c = winner_label(w, V);
    if (MODE == kModeLogits) {
      const float m = lsm_max(w.v);
      rec[t].lp = m > neg_inf() ? lsm_value(w.v, m, ctcmath::logf_normal(lsm_sum_host<DT>(probs, row0, V, m, tbl), tbl)) : neg_inf();
    } else {
      rec[t].lp = winner_lp<MODE>(w.v);
    }
  }
}

template <int DT, int MODE>
inline void greedy_item_host(const void *probs, const int32_t *seq_lens, int b, int T, int V, int blank, const uint64_t *tbl, FrameRec *rec, int32_t *tok,
                             int32_t *st, int32_t *en, float *ls, float *score, int32_t *len) {
  const int n = ctcskip::clamped_len(seq_lens, b, T);
  frame_recs_host<DT, MODE>(probs, b, T, V, n, tbl, rec);
  int L = 0;
  float sc = 0.0f, rm = 0.0f;
  for (int t = 0; t < n; ++t) {
    const int c = rec[t].c;
    sc = score_step(sc, rec[t].lp, t == 0);
    if (emits(c, t > 0 ? rec[t - 1].c : 0, t == 0, blank)) {
      tok[L] = c;
      st[L] = t;
      rm = rec[t].lp;
    } else if (c != blank) {
      rm = run_max_fwd(rm, rec[t].lp);
    }
    if (run_ends(c, t + 1 < n ? rec[t + 1].c : 0, t == n - 1, blank)) {
      if (en) en[L] = t;
      if (ls) ls[L] = rm;
      ++L;
    }
  }
  *score = sc;
  *len = L;
  for (int i = L; i < T; ++i) {
    tok[i] = st[i] = 0;
    if (en) en[i] = 0;
    if (ls) ls[i] = 0.0f;
  }
}

// One chunk call for the stream whose record is *state, item b of the call's [B, Tc, V] rows.  rec: Tc frame records (scratch); tok / st:
// Tc words each; en / ls: Tc + 1 words each and closed_len, or NULL all three; everything is written, *state included.
template <int DT, int MODE>
inline void greedy_stream_item_host(const void *probs, const int32_t *seq_lens, int b, int Tc, int V, int blank, const uint64_t *tbl, FrameRec *rec,
                                    StreamRec *state, bool eos, int32_t *tok, int32_t *st, int32_t *en, float *ls, float *score, int32_t *len,
                                    int32_t *closed_len) {
  const int n = ctcskip::clamped_len(seq_lens, b, Tc);
  frame_recs_host<DT, MODE>(probs, b, Tc, V, n, tbl, rec);
  const StreamRec r = *state;
  int E = 0, C = 0;
  float sc = r.score, rm = r.open_max;
  if (carried_closes(r, n, n > 0 ? rec[0].c : blank, eos)) {
    if (en) en[C] = stream_frame_no(r, -1);
    if (ls) ls[C] = r.open_max;
    ++C;
  }
  for (int t = 0; t < n; ++t) {
    const int c = rec[t].c;
    sc = score_step(sc, rec[t].lp, stream_first(r, t));
    if (emits(c, t > 0 ? rec[t - 1].c : rec_prev(r, blank), stream_first(r, t), blank)) {
      tok[E] = c;
      st[E] = stream_frame_no(r, t);
      ++E;
      rm = rec[t].lp;
    } else if (c != blank) {
      rm = run_max_fwd(rm, rec[t].lp);
    }
    if (stream_run_ends(c, t + 1 < n ? rec[t + 1].c : blank, t, n, eos, blank)) {
      if (en) en[C] = stream_frame_no(r, t);
      if (ls) ls[C] = rm;
      ++C;
    }
  }
  *state = stream_rec_after(r, n, n > 0 ? rec[n - 1].c : blank, E, C, sc, rm, eos, blank);
  *score = sc;
  *len = E;
  if (closed_len) *closed_len = C;
  for (int i = E; i < Tc; ++i) tok[i] = st[i] = 0;
  for (int i = C; i <= Tc; ++i) {
    if (en) en[i] = 0;
    if (ls) ls[i] = 0.0f;
  }
}

}  // namespace ctcgreedy

struct ctcd_decoder;
namespace ctcgreedy {
// what greedy.hip needs of the library's host file (ctcdecode_amd.hip) beyond align.h's hooks: the decoder's frame records, grown to `bytes`
int greedy_scratch(ctcd_decoder *d, size_t bytes, void **p);
// ... and what greedy_stream.hip needs: `bytes` of per-stream arguments of a chunk call sent to the device in one copy queued on `stream`, through
// page-locked staging the decoder owns (two slots, an event each: the call waits for nothing that is not long done); *dev: where they are
int greedy_stream_upload(ctcd_decoder *d, const void *src, size_t bytes, void *stream, void **dev);
// greedy.hip's argmax pass (in_dtype: CTCD_DTYPE_*; mode: log_input)
void launch_argmax_pass(int in_dtype, int mode, const void *probs, const int32_t *seq_lens, long long frames, int T, int V, FrameRec *rec, void *stream);
}  // namespace ctcgreedy
