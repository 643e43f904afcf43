// editops.h -- edit-operation counts and token alignments (include/ctcdecode_amd.h "Edit operations"): the Levenshtein sweep of
// editdist.h over a packed key instead of a distance.  The key of a cell is the tuple (D, S) -- edits, and substitutions among them --
// ordered lexicographically and packed as K = D * 4096 + S in one 32-bit word; the least key is the least distance and, among the
// alignments of that distance, the fewest substitutions (the most hits).  S <= min(lx, ly) <= 2048 < 4096, so the packing never
// carries, and the order of the words is the order of the tuples.
//
// What is shared with editdist.h is used from there: the lane's state (Lane<C>), the classes, the step count, where the result lands,
// the pair enumeration and the length check.  What is new here, CTC_HD and compiled for both sides like that header's routines: the
// packed cell, with and without the direction the canonical walk takes at it; a lane's start and step over keys; the layout of the
// back-pointer slot; the counts that follow from a key and two lengths; one step of the walk.  The kernels are in editops.hip, the
// sequential twin (64 simulated lanes) is at the end of this file and behind tests/native/editops_host.cpp.
//
// Roles.  The definition speaks of x and y; the schedule of the strip (the shorter row, columns c) and the streamed row (rows r).  The
// key matrix is its own transpose under exchanging x and y, so the sweep needs no role.  The walk's preference does: pair first, then
// the x-only step (an insertion), then the y-only step (a deletion).  An x-only step is a step along the strip when x is the strip and
// a step along the streamed row when it is not; `x_strip` says which, the same for a whole wave.
#pragma once
#include "editdist.h"

namespace ctcedit {

constexpr int kKeyShift = 12;
constexpr int kKeyEdit = 1 << kKeyShift;  // an insertion or a deletion: (1, 0)
constexpr int kKeySub = kKeyEdit + 1;     // a substitution: (1, 1)
constexpr int kKeyMask = kKeyEdit - 1;
constexpr int kOpsMaxDim = 1 << 18;  // the longest row: (2^18 + 1) * 4096 + 4095 < 2^31, the key and every candidate stay inside int32
constexpr long long kOpsDefaultScratch = 1ll << 30;  // ctcd_set_edit_scratch(0)

// the direction the canonical walk takes at a cell, two bits
enum : int { kDirPair = 0, kDirStream = 1 /* to (r - 1, c): the streamed token has no partner */, kDirStrip = 2 /* to (r, c - 1) */ };

// ---- the cell ----------------------------------------------------------------------------------------------------------------------
// cell_update's shape over keys: compare, add, add, min3
CTC_HD int key_cell(int up, int left, int diag, int32_t a, int32_t b) {
  int v = diag + (a != b ? kKeySub : 0);
  v = up + kKeyEdit < v ? up + kKeyEdit : v;
  return left + kKeyEdit < v ? left + kKeyEdit : v;
}
// ... and the walk's direction at the cell: the pair if it attains the key, otherwise the x-only step if it does, otherwise the y-only
CTC_HD int key_cell_dir(int up, int left, int diag, int32_t a, int32_t b, bool x_strip, int *dir) {
  const int dc = diag + (a != b ? kKeySub : 0), uc = up + kKeyEdit, lc = left + kKeyEdit;
  int v = uc < dc ? uc : dc;
  v = lc < v ? lc : v;
  const int x_only = x_strip ? lc : uc, x_dir = x_strip ? kDirStrip : kDirStream;
  *dir = dc == v ? kDirPair : (x_only == v ? x_dir : kDirStrip + kDirStream - x_dir);
  return v;
}

// ---- the counts ----------------------------------------------------------------------------------------------------------------------
// (H, S, Del, I) of every optimal alignment of rows of lx and ly tokens whose key is `key`; empty rows included: key = (lx + ly, 0)
CTC_HD void counts_of(int key, int lx, int ly, int32_t out[4]) {
  const int D = key >> kKeyShift, S = key & kKeyMask;
  const int ins = (D - S + lx - ly) / 2, del = (D - S - lx + ly) / 2;
  out[0] = lx - S - ins;
  out[1] = S;
  out[2] = del;
  out[3] = ins;
}
CTC_HD int key_trivial(int lx, int ly) { return (lx + ly) * kKeyEdit; }  // pair_trivial's answer as a key

// ---- the back-pointer slot ---------------------------------------------------------------------------------------------------------------
// A lane's C directions of a step are one word: column k of the lane at bits 2k.  32 bits for C <= 16, 64 bits for C = 32.
template <int C> struct DirWord { typedef uint32_t type; };
template <> struct DirWord<32> { typedef uint64_t type; };
// slot[row r - 1][lane], r = 1 .. m: words of the pair's class at a stride of 64 words.  A slot holds the longest streamed row the
// tensors allow in the widest word a strip of them can need -- a matter of the tensor dimensions alone.  0: no pair needs a sweep.
CTC_HD size_t ops_slot_bytes(int L, int Lq) {
  const int nmax = L < Lq ? L : Lq, rows = L < Lq ? Lq : L;
  if (nmax == 0) return 0;
  return (size_t)rows * kEditLanes * (strip_class(nmax) == 32 ? 8 : 4);
}
CTC_HD size_t slot_index(int r, int lane) { return (size_t)(r - 1) * kEditLanes + lane; }

// ---- one lane ----------------------------------------------------------------------------------------------------------------------
// Lane<C> of editdist.h, its row and its hand-offs holding keys: K[0][c] = (c, 0), K[r][0] = (r, 0)
template <int C> CTC_HD void key_lane_init(Lane<C> &L, int lane, const int32_t *strip, int n) {
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int col = lane * C + k;
    const int32_t tok = strip[col < n ? col : n - 1];
    L.a[k] = col < n ? tok : 0;
    L.prev[k] = (col + 1) * kKeyEdit;
  }
  L.diag = lane * C * kKeyEdit;
  L.tok = 0;
}
// lane_step over keys.  -> did the lane compute a row at this step?  DIRS: *word receives the directions of its C cells.
template <int C, bool DIRS>
CTC_HD bool key_lane_step(Lane<C> &L, int lane, int s, int m, int in_left, int32_t in_tok, int32_t fresh, bool x_strip, typename DirWord<C>::type *word) {
  const int r = lane_row(s, lane);
  if (r < 1 || r > m) return false;
  const int32_t t = lane == 0 ? fresh : in_tok;
  int left = lane == 0 ? r * kKeyEdit : in_left;
  int diag = L.diag;
  L.diag = left;
  L.tok = t;
  typename DirWord<C>::type w = 0;
#pragma unroll
  for (int k = 0; k < C; ++k) {
    const int up = L.prev[k];
    int v;
    if (DIRS) {
      int dir;
      v = key_cell_dir(up, left, diag, L.a[k], t, x_strip, &dir);
      w |= (typename DirWord<C>::type)dir << (2 * k);
    } else {
      v = key_cell(up, left, diag, L.a[k], t);
    }
    diag = up;
    left = v;
    L.prev[k] = v;
  }
  if (DIRS) *word = w;
  return true;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------------
// the direction stored for cell (r, c), r, c >= 1, in the word of its row and lane
template <int C> CTC_HD int dir_of(typename DirWord<C>::type w, int c) { return (int)((w >> (2 * ((c - 1) % C))) & 3); }
// One step back from (r, c), r, c >= 1, in direction dir.  A pair has partners to write: strip column c is the strip's token c - 1,
// row r the streamed token r - 1.  Then r -= walk_dr(dir), c -= walk_dc(dir).
CTC_HD void walk_pair(int r, int c, bool x_strip, int32_t *x_to_y, int32_t *y_to_x) {
  const int xi = x_strip ? c - 1 : r - 1, yi = x_strip ? r - 1 : c - 1;
  x_to_y[xi] = yi;
  y_to_x[yi] = xi;
}
CTC_HD int walk_dr(int dir) { return dir != kDirStrip ? 1 : 0; }
CTC_HD int walk_dc(int dir) { return dir != kDirStream ? 1 : 0; }
// (on the edges r == 0 or c == 0 the walk has one way to go and no partner to write: it ends there)

// ---- one pair and one call, sequentially (the host twin) -----------------------------------------------------------------------------
// key_sweep_host: sweep_host over keys; DIRS: the directions go to slot, which holds at least ops_slot_bytes of the call's dimensions
template <int C, bool DIRS> inline int key_sweep_host(const int32_t *strip, int n, const int32_t *stream, int m, bool x_strip, void *slot) {
  typedef typename DirWord<C>::type W;
  Lane<C> lanes[kEditLanes];
  for (int l = 0; l < kEditLanes; ++l) key_lane_init(lanes[l], l, strip, n);
  const int steps = sweep_steps(m, n, C), last = result_lane(n, C);
  for (int s = 0; s < steps; ++s) {
    int left[kEditLanes];
    int32_t tok[kEditLanes];
    for (int l = 0; l < kEditLanes; ++l) {
      left[l] = l > 0 ? lanes[l - 1].prev[C - 1] : 0;
      tok[l] = l > 0 ? lanes[l - 1].tok : 0;
    }
    const int32_t fresh = s < m ? stream[s] : 0;
    for (int l = 0; l < kEditLanes; ++l) {
      W w = 0;
      if (key_lane_step<C, DIRS>(lanes[l], l, s, m, left[l], tok[l], fresh, x_strip, &w) && DIRS && l <= last) ((W *)slot)[slot_index(lane_row(s, l), l)] = w;
    }
  }
  return lanes[result_lane(n, C)].prev[result_col(n, C)];
}
template <int C> inline void walk_host(const void *slot, int n, int m, bool x_strip, int32_t *x_to_y, int32_t *y_to_x) {
  typedef typename DirWord<C>::type W;
  int r = m, c = n;
  while (r > 0 && c > 0) {
    const int dir = dir_of<C>(((const W *)slot)[slot_index(r, (c - 1) / C)], c);
    if (dir == kDirPair) walk_pair(r, c, x_strip, x_to_y, y_to_x);
    r -= walk_dr(dir), c -= walk_dc(dir);
  }
}
template <int C> inline int ops_class_host(const int32_t *strip, int n, const int32_t *stream, int m, bool x_strip, bool maps, void *slot, int32_t *x_to_y, int32_t *y_to_x) {
  if (!maps) return key_sweep_host<C, false>(strip, n, stream, m, x_strip, nullptr);
  const int key = key_sweep_host<C, true>(strip, n, stream, m, x_strip, slot);
  walk_host<C>(slot, n, m, x_strip, x_to_y, y_to_x);
  return key;
}
// The key of a pair; maps: its maps too (x_to_y[0..L), y_to_x[0..Lq) are written in full), the directions going through slot.
inline int ops_pair_host(const int32_t *x, int lx, const int32_t *y, int ly, bool maps, void *slot, int32_t *x_to_y, int L, int32_t *y_to_x, int Lq) {
  if (maps) {
    for (int p = 0; p < L; ++p) x_to_y[p] = -1;
    for (int p = 0; p < Lq; ++p) y_to_x[p] = -1;
  }
  if (lx == 0 || ly == 0) return key_trivial(lx, ly);
  const bool x_strip = lx <= ly;
  const int32_t *strip = x_strip ? x : y, *stream = x_strip ? y : x;
  const int n = x_strip ? lx : ly, m = x_strip ? ly : lx;
  switch (strip_class(n)) {
    case 1: return ops_class_host<1>(strip, n, stream, m, x_strip, maps, slot, x_to_y, y_to_x);
    case 2: return ops_class_host<2>(strip, n, stream, m, x_strip, maps, slot, x_to_y, y_to_x);
    case 4: return ops_class_host<4>(strip, n, stream, m, x_strip, maps, slot, x_to_y, y_to_x);
    case 8: return ops_class_host<8>(strip, n, stream, m, x_strip, maps, slot, x_to_y, y_to_x);
    case 16: return ops_class_host<16>(strip, n, stream, m, x_strip, maps, slot, x_to_y, y_to_x);
    default: return ops_class_host<32>(strip, n, stream, m, x_strip, maps, slot, x_to_y, y_to_x);
  }
}

}  // namespace ctcedit

struct ctcd_decoder;
namespace ctcedit {
// what editops.hip needs of the library's host file beyond editdist.h's hooks: the budget of the back-pointer scratch
// (ctcd_set_edit_scratch; 0: the default), the scratch, and the slots ctcd_last_edit_slots reports
long long edit_budget(const ctcd_decoder *d);
int edit_scratch(ctcd_decoder *d, size_t bytes, void **p);
void edit_note_slots(ctcd_decoder *d, long long slots);
}  // namespace ctcedit
