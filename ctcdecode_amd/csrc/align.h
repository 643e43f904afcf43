// align.h -- CTC forced alignment (include/ctcdecode_amd.h "Forced alignment"): for every hypothesis y[0..L) of item b the best
// path of its extended sequence z (S = 2L + 1 states: z[2i] = blank, z[2i+1] = y[i]) through the item's n frames, by the Viterbi
// recurrence d[t][s] = lp(t, z[s]) + max(d[t-1][s], d[t-1][s-1], d[t-1][s-2]) in float32 -- one addition and an exact maximum per
// cell, so the result is defined bit for bit -- its score and, per label, the first and last frame the path spends on it.
//
// Everything that defines the result is CTC_HD code here, compiled for both sides: the cell update with its tie rule, the end-state
// rule, the back-pointer packing (2 bits per cell, 16 cells per word), the scratch-slot arithmetic, the back-trace step that turns a
// path into spans, and the row validation with the code it gives a row before its first frame.  The kernel of align.hip spreads a
// frame's cells over the lanes of a wave or a workgroup, by the walk of lattice_device.h that it shares with the log-likelihood
// (loglik.h, loglik.hip); align_row_host below runs them sequentially (the host twin, tests/native/align_host.cpp).  The last part
// declares what the two entry points share on the host: the decoder hooks and the entry prelude (align_entry).
//
// Every index is checked before it is followed: a length outside [0, L_stride], a label outside [0, V) or equal to the blank makes
// the row invalid -- zero outputs, score 0, the item's status word raised to ALIGN_BAD_ROW -- and never an out-of-range read.
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "blank_skip.h"
#include "exact_math_f64.h"

namespace ctcalign {

enum : int { ALIGN_BAD_ROW = 8 };  // the status word of an item with an invalid row (beam_core.h ST_* end at 6, nbest.h has 7)

constexpr int kAlignThreads = 256;                              // the kernel's workgroup: four waves of 64
constexpr int kAlignWaves = kAlignThreads / 64;
constexpr int kAlignMaxNpl = 16;                                // states one lane holds at most
constexpr int kAlignMaxStates = kAlignThreads * kAlignMaxNpl;   // 4096: the longest extended sequence one workgroup holds in registers
constexpr int kAlignMaxLabels = (kAlignMaxStates - 1) / 2;      // 2047
constexpr long long kAlignDefaultScratch = 256ll << 20;         // back-pointer scratch budget (DESIGN.md "Forced alignment")

CTC_HD float neg_inf() { return -__builtin_inff(); }

// ---- lp(t, c) --------------------------------------------------------------------------------------------------------------------
// log_input == 0: float(log(double(p) + FLT_MIN)), the value prob_to_log_kernel computes (decoder_utils.cpp:42)
CTC_HD float prob_to_lp(float p) { return (float)ctcmath::log_f64((double)p + (double)FLT_MIN, ctcmath::tables64()); }
template <int DT, bool PROB> CTC_HD float lp_at(const void *rows, size_t i) {
  const float v = ctcskip::widen_at<DT>(rows, i);
  return PROB ? prob_to_lp(v) : v;
}

// ---- the extended sequence -------------------------------------------------------------------------------------------------------
CTC_HD int n_states(int L) { return 2 * L + 1; }
CTC_HD int state_label(const int32_t *y, int s, int blank) { return (s & 1) ? y[s >> 1] : blank; }
// the third predecessor, s - 2: odd s >= 3 whose label differs from the label before it
CTC_HD bool state_skips(const int32_t *y, int s) { return (s & 1) && s >= 3 && y[s >> 1] != y[(s >> 1) - 1]; }

// ---- the cell --------------------------------------------------------------------------------------------------------------------
// The allowed predecessor with the greatest value; among equals the one with the largest state index: stay, before s - 1, before s - 2.
struct Cell {
  float v;
  unsigned bp;  // 0 stay, 1 from s - 1, 2 from s - 2
};
CTC_HD Cell cell_update(float lp, float stay, float p1, bool has1, float p2, bool has2) {
  Cell c;
  float best = stay;
  c.bp = 0u;
  if (has1 && p1 > best) { best = p1; c.bp = 1u; }
  if (has2 && p2 > best) { best = p2; c.bp = 2u; }
  c.v = lp + best;
  return c;
}
// the end state: the greater of d[n-1][S-1] and d[n-1][S-2] (S - 2 only if L >= 1); on equality S - 1
CTC_HD int end_state(int L, float d_last, float d_before) { return (L >= 1 && d_before > d_last) ? 2 * L - 1 : 2 * L; }

// ---- back-pointers: 2 bits per cell, frame t's row = bp_row_words(S) words at t * bp_row_words(S), state s in word s / 16 ----------
CTC_HD int bp_row_words(int S) { return (S + 15) >> 4; }
CTC_HD unsigned bp_shift(int s) { return 2u * ((unsigned)s & 15u); }
CTC_HD unsigned bp_get(uint32_t word, int s) { return (word >> bp_shift(s)) & 3u; }

// ---- scratch slots ---------------------------------------------------------------------------------------------------------------
// A slot holds the back-pointers of one workgroup's hypothesis in flight -- T rows of the longest extended sequence the shape allows
// (L <= min(L_stride, T): a longer row cannot be aligned and runs no recurrence) -- or of four one-wave hypotheses (S <= 64: four
// words per frame each), whichever is larger.
CTC_HD int align_lmax(int T, int L_stride) { return L_stride < T ? L_stride : T; }
CTC_HD size_t align_wave_words(int T) { return (size_t)T * 4; }  // one wave's share of a slot when four short rows run side by side
CTC_HD size_t align_slot_bytes(int T, int L_stride) {
  const size_t row = (size_t)bp_row_words(n_states(align_lmax(T, L_stride)));
  const size_t words = (size_t)T * (row > (size_t)kAlignWaves * 4 ? row : (size_t)kAlignWaves * 4);
  return (words * 4 + 255) / 256 * 256;
}
// hypotheses are classed four at a time (a group); the grid = the rows, or the slots the budget pays for, at least one (the kernel
// that runs whole groups side by side: at most the groups)
CTC_HD long long align_groups(long long rows) { return (rows + kAlignWaves - 1) / kAlignWaves; }
CTC_HD long long align_grid(long long rows, long long budget, size_t slot_bytes) {
  long long slots = (budget > 0 ? budget : kAlignDefaultScratch) / (long long)(slot_bytes ? slot_bytes : 1);
  if (slots < 1) slots = 1;
  return rows < slots ? rows : slots;
}
// states per lane of a hypothesis the whole workgroup runs
CTC_HD int align_npl(int S) { return S <= kAlignThreads ? 1 : (S <= kAlignThreads * 4 ? 4 : 16); }

// ---- row validation --------------------------------------------------------------------------------------------------------------
CTC_HD bool len_ok(int L, int L_stride) { return L >= 0 && L <= L_stride; }
CTC_HD bool label_ok(int c, int V, int blank) { return (unsigned)c < (unsigned)V && c != blank; }
// what a row is before its first frame: one of these codes, or L -- a valid row that runs the recurrence (0 <= L <= n, n >= 1)
enum : int { kRowNone = -1, kRowInvalid = -2, kRowNoPath = -3 };  // (no row; invalid; valid, but n == 0 or every label needs a frame of its own)
CTC_HD int row_code(bool ok, int len, int n) { return !ok ? kRowInvalid : ((n == 0 || len > n) ? kRowNoPath : len); }
// the score of a row that runs no recurrence (code < 0): 0 for an invalid row and for no labels in no frames, else -inf
CTC_HD float no_row_score(int code, int len, int n) { return code == kRowInvalid || (n == 0 && len == 0) ? 0.0f : neg_inf(); }
// the host twins' row, validated label by label; *n: the item's frames
inline int row_code_host(const int32_t *seq_lens, int b, int T, int V, int blank, const int32_t *tok, int len, int L_stride, int *n) {
  bool ok = len_ok(len, L_stride);
  for (int i = 0; ok && i < len; ++i) ok = label_ok(tok[i], V, blank);
  *n = ctcskip::clamped_len(seq_lens, b, T);
  return row_code(ok, len, *n);
}

// ---- the back-trace --------------------------------------------------------------------------------------------------------------
// The path is in state e at frame n - 1 ...
CTC_HD void trace_begin(int e, int n, int32_t *en, bool write) {
  if (write && (e & 1)) en[e >> 1] = n - 1;
}
// ... in state s at frame t >= 1 with back-pointer bp: returns its state at t - 1.  A label's span starts where the path enters its
// state and ends where it leaves it.  (bp <= s for every pointer cell_update records; the clamp keeps a wrong word inside the row.)
CTC_HD int trace_step(int s, unsigned bp, int t, int32_t *st, int32_t *en, bool write) {
  if (bp > (unsigned)s) bp = (unsigned)s;
  if (bp) {
    if (write && (s & 1)) st[s >> 1] = t;
    s -= (int)bp;
    if (write && (s & 1)) en[s >> 1] = t - 1;
  }
  return s;
}
// ... and in state s at frame 0
CTC_HD void trace_end(int s, int32_t *st, bool write) {
  if (write && (s & 1)) st[s >> 1] = 0;
}

// ---- one hypothesis, sequentially (the host twin) ----------------------------------------------------------------------------------
// Row `tok` (L_stride words, `len` of them labels) of item b against the item's rows; slot: align_slot_bytes(T, L_stride) bytes of
// scratch.  st / en: L_stride words each, all written.  Returns 0, or ALIGN_BAD_ROW.
template <int DT, bool PROB>
inline int align_row_host(const void *probs, const int32_t *seq_lens, int b, int T, int V, int blank, const int32_t *tok, int len, int L_stride, uint32_t *slot,
                          int32_t *st, int32_t *en, float *score) {
  for (int i = 0; i < L_stride; ++i) st[i] = en[i] = 0;
  int n;
  const int L = row_code_host(seq_lens, b, T, V, blank, tok, len, L_stride, &n), S = n_states(L);
  if (L < 0) {
    *score = no_row_score(L, len, n);
    return L == kRowInvalid ? ALIGN_BAD_ROW : 0;
  }
  const int wpf = bp_row_words(S);
  const size_t row0 = (size_t)b * T;
  std::vector<float> d((size_t)S), nd((size_t)S);
  for (int s = 0; s < S; ++s) d[(size_t)s] = s < 2 ? lp_at<DT, PROB>(probs, row0 * V + (size_t)state_label(tok, s, blank)) : neg_inf();
  for (int t = 1; t < n; ++t) {
    uint32_t *row = slot + (size_t)t * wpf;
    for (int w = 0; w < wpf; ++w) row[w] = 0u;
    for (int s = 0; s < S; ++s) {
      const float lp = lp_at<DT, PROB>(probs, (row0 + (size_t)t) * V + (size_t)state_label(tok, s, blank));
      const Cell c = cell_update(lp, d[(size_t)s], s >= 1 ? d[(size_t)s - 1] : 0.0f, s >= 1, s >= 2 ? d[(size_t)s - 2] : 0.0f, state_skips(tok, s));
      nd[(size_t)s] = c.v;
      row[s >> 4] |= c.bp << bp_shift(s);
    }
    d.swap(nd);
  }
  const int e = end_state(L, d[(size_t)S - 1], L >= 1 ? d[(size_t)S - 2] : 0.0f);
  *score = d[(size_t)e];
  if (!(*score > neg_inf()) || L == 0) return 0;  // not aligned (spans 0), or nothing to place
  trace_begin(e, n, en, true);
  int s = e;
  for (int t = n - 1; t >= 1; --t) s = trace_step(s, bp_get(slot[(size_t)t * wpf + (s >> 4)], s), t, st, en, true);
  trace_end(s, st, true);
  return 0;
}

// ---- what align.hip needs of the library's host file (ctcdecode_amd.hip) ------------------------------------------------------------
struct AlignDecoderInfo {
  int device;
  int in_dtype;
  long long budget;  // ctcd_set_align_scratch (0: the default)
};

}  // namespace ctcalign

struct ctcd_decoder;
namespace ctcdev {
struct DeviceGuard;  // device_guard.h
}
namespace ctcalign {
// What ctcd_ctc_align and ctcd_ctc_loglik do alike before their launch (align.hip): the checks of the arguments they share -- `fn`, the
// entry point's name, stands in the messages; `outputs`: its output tensors are there -- the decoder's info, its device entered
// through `guard`, and for raw logits the log-softmax pass.  -> CTCD_OK with e filled in (rows == 0: nothing to do), or the failure.
struct AlignEntry {
  long long rows;     // B * R
  const void *probs;  // the rows to read, of element type `dtype`, log-probabilities unless log_input == 0
  int dtype;
  AlignDecoderInfo inf;
};
int align_entry(const char *fn, ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *tokens,
                const int32_t *lens, int R, int L_stride, bool outputs, void *stream, ctcdev::DeviceGuard *guard, AlignEntry *e);
int align_decoder_info(const ctcd_decoder *d, AlignDecoderInfo *out);
int align_fail(int code, const char *msg);
// the decoder's back-pointer scratch, grown to `bytes`
int align_scratch(ctcd_decoder *d, size_t bytes, void **p);
// raw logits: the log-softmax pass (ctcd_log_softmax) into decoder-owned float32 rows
int align_lsm_rows(ctcd_decoder *d, const void *logits, const int32_t *seq_lens, int B, int T, int V, void *stream, const float **rows);
void align_note_grid(ctcd_decoder *d, long long grid);  // ctcd_last_align_grid
}  // namespace ctcalign
