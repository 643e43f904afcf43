// editdist.h -- Levenshtein distances between label rows (include/ctcdecode_amd.h "Edit distance"): unit costs, int32 tokens compared
// as values, integer arithmetic throughout -- so the result is exact and equality is equality.
//
// Everything that is not a launch is CTC_HD code here, compiled for both sides: the cell update, the lane-strip schedule (one lane's
// state, its start, one step of it), where the result lands and after how many steps, the class function, the enumeration of the pairs
// of a call in both modes, and the validation of an item's lengths.  The kernel of editdist.hip gives a pair to a wave and lets the 64
// lanes step side by side, the hand-off between neighbours a one-lane shift; pair_host below steps 64 simulated lanes one after the
// other (the host twin, tests/native/editdist_host.cpp).
//
// The schedule.  Of a pair's two rows the shorter is the STRIP a[0..n), the longer is STREAMED s[0..m): lev is symmetric, so the choice
// is free, and it keeps the limit a matter of tensor dimensions.  D[r][c], r = 0..m, c = 0..n, is the distance between s[0..r) and
// a[0..c); D[0][c] = c, D[r][0] = r.  Lane l owns the columns l*C + 1 .. (l+1)*C: their tokens and its current row of D stay in
// registers.  At step s = 0, 1, .. lane l computes row r = s - l + 1 (if 1 <= r <= m): a wavefront that runs down the anti-diagonals of
// the lanes.  What lane l needs from outside is column l*C of rows r and r - 1: lane l - 1 computed the first at step s - 1 -- it hands
// over its last column after every step -- and the second is what it handed over the step before, which lane l has kept.  Lane 0's
// left edge is the row number.  The streamed token travels the same way: lane 0 takes s[r - 1] fresh, lane l takes the token lane
// l - 1 used the step before.  Columns beyond n are computed and never looked at (a cell depends on nothing to its right).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef CTC_HD
#if defined(__HIPCC__)
#define CTC_HD __host__ __device__ __forceinline__
#else
#define CTC_HD inline
#endif
#endif

namespace ctcedit {

enum : int { EDIT_BAD_ROW = 8 };  // the status word of an item with a length outside its bounds: CTCD_ALIGN_BAD_ROW, the same meaning

constexpr int kEditLanes = 64;                         // a wave
constexpr int kEditMaxC = 32;                          // columns one lane holds at most
constexpr int kEditMaxStrip = kEditLanes * kEditMaxC;  // 2048: the longest strip
constexpr int kEditThreads = 256;                      // the kernel's workgroup: four waves, four pairs
constexpr int kEditWaves = kEditThreads / kEditLanes;
constexpr int kEditMaxDim = 1 << 30;                   // the longest row stride: step numbers stay well inside int32
constexpr int kEditWavesPerCu = 8;                     // the persistent grid: two workgroups of four waves per compute unit (the kernel's registers allow two waves per SIMD)

// ---- the cell ----------------------------------------------------------------------------------------------------------------------
// D[r][c] from D[r-1][c] (up), D[r][c-1] (left) and D[r-1][c-1] (diag): insertion, deletion and substitution cost 1, a match 0
CTC_HD int cell_update(int up, int left, int diag, int32_t a, int32_t b) {
  int v = diag + (a != b ? 1 : 0);
  v = up + 1 < v ? up + 1 : v;
  return left + 1 < v ? left + 1 : v;
}

// ---- the classes -------------------------------------------------------------------------------------------------------------------
// Columns per lane, a compile-time constant of the sweep: the least power of two C with 64 * C >= n, for a strip of 1 <= n <= 2048
// tokens.  (A pair costs about (m + n / C) steps of C cells: a strip of 250 labels in class 4 does an eighth of class 32's work.)
constexpr int kEditClasses[] = {1, 2, 4, 8, 16, 32};
constexpr int kEditNumClasses = 6;
CTC_HD int strip_class(int n) {
  int c = 1;
  while (kEditLanes * c < n) c <<= 1;
  return c;
}

// ---- where the result lands --------------------------------------------------------------------------------------------------------
// D[m][n] is column (n - 1) % C of lane (n - 1) / C, once that lane has finished row m: after sweep_steps steps (n >= 1)
CTC_HD int result_lane(int n, int C) { return (n - 1) / C; }
CTC_HD int result_col(int n, int C) { return (n - 1) % C; }
CTC_HD int sweep_steps(int m, int n, int C) { return m + result_lane(n, C); }
// the row lane `lane` computes at step s; rows outside 1 .. m are not computed
CTC_HD int lane_row(int s, int lane) { return s - lane + 1; }
// the empty cases need no sweep: lev(a, []) = len(a)
CTC_HD bool pair_trivial(int lx, int ly, int *dist) {
  if (lx != 0 && ly != 0) return false;
  *dist = lx + ly;
  return true;
}

// ---- one lane ----------------------------------------------------------------------------------------------------------------------
template <int C> struct Lane {
  int32_t a[C];  // the strip's tokens of the lane's columns (0 beyond the strip: nothing at or beyond n is read)
  int prev[C];   // the lane's latest row of D over its columns; prev[C - 1] is what it hands to lane + 1
  int diag;      // column lane * C of the row before the next one to compute
  int32_t tok;   // the streamed token of the lane's latest row: what it hands to lane + 1
};
template <int C> CTC_HD void lane_init(Lane<C> &L, int lane, const int32_t *strip, int n) {
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int col = lane * C + k;  // 0-based token index; D's column col + 1
    const int32_t tok = strip[col < n ? col : n - 1];  // (an index inside the row whatever the column: the loads need no branch)
    L.a[k] = col < n ? tok : 0;
    L.prev[k] = col + 1;  // row 0
  }
  L.diag = lane * C;
  L.tok = 0;
}
// Step s.  in_left / in_tok: prev[C - 1] and tok of lane - 1 as they stood BEFORE this step (lane 0: ignored); fresh: the streamed
// token of row s + 1 (lane 0 alone looks at it).
template <int C> CTC_HD void lane_step(Lane<C> &L, int lane, int s, int m, int in_left, int32_t in_tok, int32_t fresh) {
  const int r = lane_row(s, lane);
  if (r < 1 || r > m) return;
  const int32_t t = lane == 0 ? fresh : in_tok;
  int left = lane == 0 ? r : in_left;
  int diag = L.diag;
  L.diag = left;
  L.tok = t;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int up = L.prev[k];
    const int v = cell_update(up, left, diag, L.a[k], t);
    diag = up;
    left = v;
    L.prev[k] = v;
  }
}

// ---- the pairs of a call -----------------------------------------------------------------------------------------------------------
// General mode: B * R * Q pairs, pair w = (b, i, j) row-major.  Pairwise mode (y == x, Q == R): the B * R * (R - 1) / 2 pairs i < j,
// an item's pairs in the order (0,1) (0,2) .. (0,R-1) (1,2) ..; the diagonal is written apart.
struct Pair {
  int b, i, j;
};
CTC_HD long long pairs_per_item(int R, int Q, bool pairwise) { return pairwise ? (long long)R * (R - 1) / 2 : (long long)R * Q; }
// the pairs (i', j) with i' < i: rows 0 .. i - 1 hold R - 1, R - 2, .. pairs
CTC_HD long long triangle_offset(long long i, int R) { return i * (2ll * R - i - 1) / 2; }
CTC_HD Pair pair_of(long long w, int R, int Q, bool pairwise) {
  const long long per = pairs_per_item(R, Q, pairwise);
  Pair p;
  p.b = (int)(w / per);
  const long long k = w - (long long)p.b * per;
  if (!pairwise) {
    p.i = (int)(k / Q);
    p.j = (int)(k - (long long)p.i * Q);
    return p;
  }
  // the row i with triangle_offset(i) <= k < triangle_offset(i + 1): a floating-point estimate, settled by integer steps
  const double t = 2.0 * R - 1.0, disc = t * t - 8.0 * (double)k;
  long long i = (long long)((t - __builtin_sqrt(disc > 0.0 ? disc : 0.0)) * 0.5);
  if (i < 0) i = 0;
  if (i > R - 2) i = R - 2;
  while (i > 0 && triangle_offset(i, R) > k) --i;
  while (i < R - 2 && triangle_offset(i + 1, R) <= k) ++i;
  p.i = (int)i;
  p.j = (int)(i + 1 + (k - triangle_offset(i, R)));
  return p;
}

// ---- the validation ----------------------------------------------------------------------------------------------------------------
CTC_HD bool len_ok(int len, int L) { return len >= 0 && len <= L; }

// ---- one pair and one call, sequentially (the host twin) -----------------------------------------------------------------------------
// 64 simulated lanes, stepped one after the other from a snapshot of what their neighbours hand over
template <int C> inline int sweep_host(const int32_t *strip, int n, const int32_t *stream, int m) {
  Lane<C> lanes[kEditLanes];
  for (int l = 0; l < kEditLanes; ++l) lane_init(lanes[l], l, strip, n);
  const int steps = sweep_steps(m, n, C);
  for (int s = 0; s < steps; ++s) {
    int left[kEditLanes];
    int32_t tok[kEditLanes];
    for (int l = 0; l < kEditLanes; ++l) {
      left[l] = l > 0 ? lanes[l - 1].prev[C - 1] : 0;
      tok[l] = l > 0 ? lanes[l - 1].tok : 0;
    }
    const int32_t fresh = s < m ? stream[s] : 0;
    for (int l = 0; l < kEditLanes; ++l) lane_step(lanes[l], l, s, m, left[l], tok[l], fresh);
  }
  return lanes[result_lane(n, C)].prev[result_col(n, C)];
}
inline int pair_host(const int32_t *x, int lx, const int32_t *y, int ly) {
  int d;
  if (pair_trivial(lx, ly, &d)) return d;
  const bool x_strip = lx <= ly;
  const int32_t *strip = x_strip ? x : y, *stream = x_strip ? y : x;
  const int n = x_strip ? lx : ly, m = x_strip ? ly : lx;
  switch (strip_class(n)) {
    case 1: return sweep_host<1>(strip, n, stream, m);
    case 2: return sweep_host<2>(strip, n, stream, m);
    case 4: return sweep_host<4>(strip, n, stream, m);
    case 8: return sweep_host<8>(strip, n, stream, m);
    case 16: return sweep_host<16>(strip, n, stream, m);
    default: return sweep_host<32>(strip, n, stream, m);
  }
}
// are all lengths of item b inside their bounds?  (y == NULL: pairwise mode)
inline bool item_ok_host(const int32_t *x_lens, int b, int R, int L, const int32_t *y_lens, int Q, int Lq) {
  bool ok = true;
  for (int i = 0; i < R; ++i) ok = ok && len_ok(x_lens[(size_t)b * R + i], L);
  if (y_lens)
    for (int j = 0; j < Q; ++j) ok = ok && len_ok(y_lens[(size_t)b * Q + j], Lq);
  return ok;
}
// the whole contract for checked arguments (B, R, Q >= 1); *pairs: the sweeps and trivial answers it ran
inline int edit_distance_host(const int32_t *x, const int32_t *x_lens, int B, int R, int L, const int32_t *y, const int32_t *y_lens, int Q, int Lq, int32_t *out,
                              int32_t *status, long long *pairs) {
  const bool pairwise = y == nullptr;
  if (pairwise) Q = R, Lq = L;
  const long long per = pairs_per_item(R, Q, pairwise), work = per * B;
  *pairs = work;
  for (long long w = 0; w < work; ++w) {
    const Pair p = pair_of(w, R, Q, pairwise);
    int d = 0;
    if (item_ok_host(x_lens, p.b, R, L, pairwise ? nullptr : y_lens, Q, Lq)) {
      const int32_t *xr = x + ((size_t)p.b * R + p.i) * L, *yr = pairwise ? x + ((size_t)p.b * R + p.j) * L : y + ((size_t)p.b * Q + p.j) * Lq;
      d = pair_host(xr, x_lens[(size_t)p.b * R + p.i], yr, pairwise ? x_lens[(size_t)p.b * R + p.j] : y_lens[(size_t)p.b * Q + p.j]);
    } else if (status) {
      status[p.b] = EDIT_BAD_ROW;
    }
    out[((size_t)p.b * R + p.i) * Q + p.j] = d;
    if (pairwise) out[((size_t)p.b * R + p.j) * Q + p.i] = d;
  }
  if (pairwise)
    for (long long k = 0; k < (long long)B * R; ++k) {
      const int b = (int)(k / R), i = (int)(k % R);
      out[((size_t)b * R + i) * R + i] = 0;
      if (status && !item_ok_host(x_lens, b, R, L, nullptr, Q, Lq)) status[b] = EDIT_BAD_ROW;
    }
  return 0;
}

}  // namespace ctcedit

struct ctcd_decoder;
namespace ctcedit {
// what editdist.hip needs of the library's host file (ctcdecode_amd.hip): the decoder's device and compute units, ctcd_last_error,
// the cap of the grid, and the counts ctcd_last_edit_pairs and ctcd_last_edit_grid report
struct EditDecoderInfo {
  int device;
  int cus;
  long long cap;  // ctcd_set_edit_grid (0: the default)
};
int edit_decoder_info(const ctcd_decoder *d, EditDecoderInfo *out);
int edit_fail(int code, const char *msg);
void edit_note_pairs(ctcd_decoder *d, long long pairs, long long grid);  // ctcd_last_edit_pairs, ctcd_last_edit_grid
}  // namespace ctcedit
