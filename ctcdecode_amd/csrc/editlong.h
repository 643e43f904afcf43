// editlong.h -- edit distances and edit counts of pairs whose SHORTER row is beyond one wave's registers (include/ctcdecode_amd.h
// "Long edit pairs", ctcd_set_edit_long): one workgroup of W waves per pair, the parallelism found inside the pair.
//
// Tiles.  The strip a[0..n) of editdist.h is cut into tiles of 2048 columns, tile k = columns 2048 k + 1 .. 2048 (k + 1); the streamed
// row s[0..m), m >= n, runs past every tile.  A wave sweeps a tile exactly as sweep<32> of editdist.hip sweeps a whole strip -- Lane<32>,
// lane_init with the tile's column offset, lane_step<32, true> -- with two differences at the edges: lane 0's left edge of row r is
// D[r][2048 k], which the wave of tile k - 1 hands over (tile 0: the row number), and lane 63 hands D[r][2048 (k + 1)] on after every row.
// Columns beyond n in the last tile are computed and never read, as in editdist.h; the tiles are not balanced.
//
// The schedule has one definition, the functions below, used by the kernel (editlong.hip) and by the sequential twin at the end:
//   * Time runs in BLOCKS of 64 steps, a workgroup barrier after each.  A tile takes long_tile_blocks(m) blocks: m + 63 steps.
//   * Wave w sweeps tiles w, w + W, w + 2W, ..: tile k = rho W + w in ROUND rho.  It runs the tile's block j in the global block
//     rho P + 2 w + j, P = long_period: a tile runs kLongLag = 2 blocks behind its left neighbour.  Why two: lane 63 finishes row r at
//     the tile's step r + 62, so once block j has ended rows up to 64 j + 1 are complete (long_rows_done); lane 0 of the next tile needs
//     rows 64 j + 1 .. 64 j + 64 during ITS block j, so everything up to 64 j + 64 must have been complete a barrier earlier: the
//     neighbour must have ended its block j + 1.  One block of lag leaves row 64 j + 2 .. unfinished, two are enough.
//   * P = max(blocks of a tile + kLongLag, 2 W).  2 W: tile rho W - 1 (wave W - 1, 2 (W - 1) blocks behind wave 0) has ended the block
//     wave 0 needs before wave 0 starts tile rho W.  Blocks + 2: a wave's ring outlives its tile by the lag -- the right neighbour
//     reads it up to 2 blocks after the tile's last block -- so the wave idles those 2 blocks (of 33 or more: m > 2048) before its next
//     tile's lane 63 stores row 1 at that ring's index 1.
//   * Inside a round an edge travels through an LDS ring per wave boundary, kLongRing = 256 values, row r at r mod 256.  While the
//     consumer reads rows 64 j + 1 .. 64 j + 64 at the top of a block, its producer writes rows 64 j + 66 .. 64 j + 129 in that block:
//     129 rows are alive at once, and 256 is the next power of two.
//     THE RING'S INVARIANT: between the block that stores row r of tile k and the block in which tile k + 1 loads it, that block
//     included, nothing else is stored at index r mod 256 of that ring.  Row r + 256 of tile k is stored 2 blocks or more after
//     the load (block (r + 318) / 64 of tile k against block (r - 1) / 64 + 2); tile k + W starts P >= blocks + 2 after tile k, and
//     tile k + 1 loads its last row in block blocks + 1 after tile k's start.
//   * Between rounds up to m edges wait: they go through a column of m + 1 values in decoder-owned scratch (the workgroup's SLOT),
//     written by wave W - 1 with plain vector stores, read by wave 0 a round later; a device-scope fence stands in front of every
//     barrier.  Wave W - 1 overwrites row r in the next round 2 (W - 1) blocks after wave 0 has read it.
//   * The streamed token is read again from global memory by every tile (64 tokens a block ahead, as sweep<32> does), it does not
//     travel with the edge.
//
// The cell policy.  Distance (DistCell): one word per cell, Lane<32> and lane_step as they are.  Counts (CountCell): the tuple (D, S) of
// editops.h as ONE 64-bit key D * 2^32 + S -- S can exceed the 4095 of the packed 32-bit key here -- with the same lexicographic
// minimum; counts_of_ds takes D and S apart.  Limits: a long pair needs D < 2^31, which the 2^30 positions of a row give; the
// packed key and its max(L, Lq) <= 262144 hold for calls with the mode off and, with it on, for nothing: a pair whose streamed row is
// beyond 262144 goes to this kernel whatever its strip.
//
// Alignments (AlignCell, ctcd_edit_align with the mode on).  Two bits per cell of 30000 x 30000 are 225 MB, so the long kernel keeps
// CHECKPOINTS of the key matrix instead and recovers the canonical walk from them, in memory that grows with m + n:
//   * The forward pass is the CountCell sweep above with two additions.  Lane 63 stores its right edge K[r][2048 (k + 1)] of EVERY
//     tile but the last, on every wave, into a column per tile of the workgroup's slot (the column checkpoints; they subsume the column
//     between rounds: wave 0 reads its left edge from the checkpoint of tile k - 1).  And every lane stores the 32 keys of its row
//     when its row number is a multiple of kAlignBand = 1024 (the row checkpoints).  Row 0 and column 0 are closed forms.
//   * The walk runs behind the pair's last block, on wave 0, from (r, c) = (m, n), BLOCK by block: tile (c - 1) / 2048 x band
//     (r - 1) / 1024.  The wave sweeps the block again from the row checkpoint above it and the column checkpoint to its left, up to row
//     r and lane column (c - 1) / 32 only, with the direction of key64_cell_dir per cell -- editops.h's rule over 64-bit keys -- one
//     64-bit word per lane and row into the slot's block buffer of 1024 x 64 words, then walks as editops.hip's kernel does until it
//     leaves the block by its top row or its left column.  Partners are written with global indices (walk_pair).
//   * The slot, from the tensor dimensions alone (long_align_slot_bytes): tiles(min) x (max + 1) keys of column checkpoints,
//     (max / 1024) x tiles(min) x 2048 keys of row checkpoints, the block buffer of 512 KiB.  11.2 MB at 30000 x 30000.
// Not here: alignments in pairwise mode, weighted costs, several workgroups on one pair, the idle W - 1 waves during the walk.
#pragma once
#include "editops.h"

namespace ctcedit {

constexpr int kLongTile = kEditMaxStrip;  // columns of a tile: a wave's registers, 64 lanes x 32 columns
constexpr int kLongC = kEditMaxC;
constexpr int kLongBlock = kEditLanes;    // steps between two barriers
constexpr int kLongLag = 2;               // blocks a tile runs behind its left neighbour
constexpr int kLongRing = 256;            // values of an LDS ring
constexpr int kLongMaxWaves = 16;
constexpr int kLongDefaultWaves = 16;     // what ctcd_set_edit_long's callers pass by default
constexpr int kLongSlotAlign = 256;

CTC_HD bool long_waves_ok(int w) { return w == 2 || w == 4 || w == 8 || w == 16; }

// ---- the schedule --------------------------------------------------------------------------------------------------------------------
CTC_HD int long_tiles(int n) { return (n + kLongTile - 1) / kLongTile; }
CTC_HD int long_tile_steps(int m) { return m + kEditLanes - 1; }  // lane 63 computes row m at step m + 62
CTC_HD int long_tile_blocks(int m) { return (long_tile_steps(m) + kLongBlock - 1) / kLongBlock; }
CTC_HD int long_period(int m, int W) {
  const int nb = long_tile_blocks(m);  // (+ kLongLag: the ring's invariant above)
  return nb + kLongLag > kLongLag * W ? nb + kLongLag : kLongLag * W;
}
// the global blocks of a pair: the last tile ends last
CTC_HD long long long_blocks(int m, int n, int W) {
  const int last = long_tiles(n) - 1;
  return (long long)(last / W) * long_period(m, W) + kLongLag * (last % W) + long_tile_blocks(m);
}
// what wave w does in global block g: nothing, or block `block` of tile `tile`
struct LongSlot {
  bool active;
  int tile, block;
};
CTC_HD LongSlot long_slot(long long g, int w, int m, int n, int W) {
  LongSlot s = {false, 0, 0};
  const long long t = g - kLongLag * w;
  if (t < 0) return s;
  const int P = long_period(m, W);
  const long long round = t / P;
  s.block = (int)(t - round * P);
  const long long tile = round * W + w;
  if (s.block >= long_tile_blocks(m) || tile >= long_tiles(n)) return s;
  s.tile = (int)tile;
  s.active = true;
  return s;
}
// the rows lane 0 of a tile takes its left edge of during the tile's block j: row_first .. row_first + 63 (those up to m)
CTC_HD int long_row_first(int j) { return j * kLongBlock + 1; }
// the rows whose right edge is complete once a tile's block j has ended: 1 .. long_rows_done (at most m)
CTC_HD int long_rows_done(int j, int m) {
  const int r = (j + 1) * kLongBlock - (kEditLanes - 1);
  return r < m ? r : m;
}
// the row lane 63 completes at step s (outside 1 .. m: none)
CTC_HD int long_edge_row(int s) { return s - (kEditLanes - 2); }
CTC_HD int long_ring_index(int r) { return r & (kLongRing - 1); }
// the slot: the column between two rounds, max(L, Lq) + 1 values -- a matter of the tensor dimensions alone
CTC_HD size_t long_slot_bytes(int L, int Lq, bool counts) {
  const size_t rows = (size_t)(L < Lq ? Lq : L) + 1, bytes = rows * (counts ? 8 : 4);
  return (bytes + kLongSlotAlign - 1) / kLongSlotAlign * kLongSlotAlign;
}
// which pairs of a call with the mode on leave the per-wave kernel for this one
CTC_HD bool long_pair(int n, int m, bool counts) { return n > kEditMaxStrip || (counts && m > kOpsMaxDim); }

// ---- the cell policies ---------------------------------------------------------------------------------------------------------------
struct DistCell {
  typedef int V;
  typedef Lane<kLongC> L;
  static constexpr bool kCounts = false;
  static constexpr bool kCheckpoints = false;
  static CTC_HD V edge0(int r) { return r; }  // D[r][0]
  static CTC_HD V last(const L &l) { return l.prev[kLongC - 1]; }
  static CTC_HD void init(L &l, int lane, const int32_t *strip, int n, int col0) { lane_init(l, lane, strip, n, col0); }
  static CTC_HD void step(L &l, int lane, int s, int m, V in_left, int32_t in_tok, int32_t fresh) {
    lane_step<kLongC, true>(l, lane, s, m, in_left, in_tok, fresh);
  }
  // (H, S, Del, I) are not a distance's business: out is one word
  static CTC_HD void result(V v, int, int, int32_t *out, int32_t *mirror) {
    out[0] = v;
    if (mirror) mirror[0] = v;
  }
  static constexpr int kOutWords = 1;
};

constexpr long long kKey64Edit = 1ll << 32;       // an insertion or a deletion: (1, 0)
constexpr long long kKey64Sub = kKey64Edit + 1;   // a substitution: (1, 1)
// key_cell's shape over 64-bit keys
CTC_HD long long key64_cell(long long up, long long left, long long diag, int32_t a, int32_t b) {
  long long v = diag + (a != b ? kKey64Sub : 0);
  v = up + kKey64Edit < v ? up + kKey64Edit : v;
  return left + kKey64Edit < v ? left + kKey64Edit : v;
}
struct KeyLane64 {  // Lane<32> with a row of 64-bit keys
  int32_t a[kLongC];
  long long prev[kLongC];
  long long diag;
  int32_t tok;
};
struct CountCell {
  typedef long long V;
  typedef KeyLane64 L;
  static constexpr bool kCounts = true;
  static constexpr bool kCheckpoints = false;
  static CTC_HD V edge0(int r) { return (long long)r * kKey64Edit; }
  static CTC_HD V last(const L &l) { return l.prev[kLongC - 1]; }
  static CTC_HD void init(L &l, int lane, const int32_t *strip, int n, int col0) {
#pragma unroll
    for (int k = 0; k < kLongC; ++k) {
      const int col = col0 + lane * kLongC + k;
      const int32_t tok = strip[col < n ? col : n - 1];
      l.a[k] = col < n ? tok : 0;
      l.prev[k] = (long long)(col + 1) * kKey64Edit;
    }
    l.diag = (long long)(col0 + lane * kLongC) * kKey64Edit;
    l.tok = 0;
  }
  // lane_step<32, true> over 64-bit keys
  static CTC_HD void step(L &l, int lane, int s, int m, V in_left, int32_t in_tok, int32_t fresh) {
    const int r = lane_row(s, lane);
    if (r < 1 || r > m) return;
    const int32_t t = lane == 0 ? fresh : in_tok;
    long long left = in_left, diag = l.diag;
    l.diag = left;
    l.tok = t;
#pragma unroll
    for (int k = 0; k < kLongC; ++k) {
      const long long up = l.prev[k];
      const long long v = key64_cell(up, left, diag, l.a[k], t);
      diag = up;
      left = v;
      l.prev[k] = v;
    }
  }
  // in x / y terms, like edit_counts_kernel; the mirror (pairwise mode) has deletions and insertions exchanged
  static CTC_HD void result(V v, int lx, int ly, int32_t *out, int32_t *mirror) {
    int32_t c[4];
    counts_of_ds((int)(v >> 32), (int)(v & 0xffffffffll), lx, ly, c);
    out[0] = c[0], out[1] = c[1], out[2] = c[2], out[3] = c[3];
    if (mirror) mirror[0] = c[0], mirror[1] = c[1], mirror[2] = c[3], mirror[3] = c[2];
  }
  static constexpr int kOutWords = 4;
};
// the value of a tile's local column col (0 .. 31) of lane's row: a select chain, the row stays in registers.  (A recursion, not a
// loop: the compiler rewrites the loop's exit value into an indexed load, and the row then lives in scratch memory for that one load.)
template <class P, int K> struct LongPick {
  static CTC_HD typename P::V get(const typename P::L &l, int col) {
    const typename P::V v = LongPick<P, K - 1>::get(l, col);
    return K == col ? l.prev[K] : v;
  }
};
template <class P> struct LongPick<P, 0> {
  static CTC_HD typename P::V get(const typename P::L &l, int) { return l.prev[0]; }
};
template <class P> CTC_HD typename P::V long_pick(const typename P::L &l, int col) { return LongPick<P, kLongC - 1>::get(l, col); }

// ---- alignments: the checkpoints, the slot, a block's sweep --------------------------------------------------------------------------
constexpr int kAlignBand = 1024;  // rows between two row checkpoints: the rows of a block (its columns: a tile's, kLongTile)
struct AlignCell : CountCell {    // the CountCell sweep that also keeps the checkpoints
  static constexpr bool kCheckpoints = true;
};
// a slot's three parts; a pair of (n, m) tokens uses tiles(n) <= tiles and m <= rows of them
struct AlignSlot {
  long long *colck;  // [tiles][rows + 1]: K[r][2048 (k + 1)] at (k, r), r = 1 .. m, k = 0 .. tiles(n) - 2
  long long *rowck;  // [rows / 1024][tiles][2048]: K[r][2048 k + 1 + col] at (r, k, col), r = 1024, 2048, .. <= m
  uint64_t *dirs;    // [1024][64]: the directions of the block the walk stands in, a word per row and lane
  int tiles, rows;
};
CTC_HD int align_slot_tiles(int L, int Lq) { return long_tiles(L < Lq ? L : Lq); }
CTC_HD int align_slot_rows(int L, int Lq) { return L < Lq ? Lq : L; }
CTC_HD size_t align_col_words(int L, int Lq) { return (size_t)align_slot_tiles(L, Lq) * ((size_t)align_slot_rows(L, Lq) + 1); }
CTC_HD size_t align_row_words(int L, int Lq) { return (size_t)(align_slot_rows(L, Lq) / kAlignBand) * align_slot_tiles(L, Lq) * kLongTile; }
constexpr size_t kAlignDirWords = (size_t)kAlignBand * kEditLanes;
// the slot of a long alignment -- a matter of the tensor dimensions alone
CTC_HD size_t long_align_slot_bytes(int L, int Lq) {
  const size_t bytes = (align_col_words(L, Lq) + align_row_words(L, Lq) + kAlignDirWords) * 8;
  return (bytes + kLongSlotAlign - 1) / kLongSlotAlign * kLongSlotAlign;
}
CTC_HD AlignSlot align_slot(char *base, int L, int Lq) {
  AlignSlot s;
  s.colck = (long long *)base;
  s.rowck = s.colck + align_col_words(L, Lq);
  s.dirs = (uint64_t *)(s.rowck + align_row_words(L, Lq));
  s.tiles = align_slot_tiles(L, Lq), s.rows = align_slot_rows(L, Lq);
  return s;
}
CTC_HD size_t align_col_index(const AlignSlot &s, int k, int r) { return (size_t)k * ((size_t)s.rows + 1) + r; }
// (r: a multiple of kAlignBand, 1024 or more)
CTC_HD size_t align_row_index(const AlignSlot &s, int r, int k, int col) { return ((size_t)(r / kAlignBand - 1) * s.tiles + k) * kLongTile + col; }
CTC_HD size_t align_dir_index(int local_row, int lane) { return (size_t)(local_row - 1) * kEditLanes + lane; }  // local_row = 1 .. 1024
// the slot of the per-wave kernel in a call with the mode on: the pairs it keeps have a strip of 2048 columns and a streamed row of
// 262144 tokens at the most
CTC_HD size_t long_short_slot_bytes(int L, int Lq) {
  const int rows = align_slot_rows(L, Lq);
  return (size_t)(rows < kOpsMaxDim ? rows : kOpsMaxDim) * kEditLanes * 8;
}
// the block the walk stands in at (r, c), r, c >= 1: its tile, and the row above its first
CTC_HD int align_tile_of(int c) { return (c - 1) / kLongTile; }
CTC_HD int align_row0_of(int r) { return (r - 1) / kAlignBand * kAlignBand; }

// key_cell_dir over 64-bit keys
CTC_HD long long key64_cell_dir(long long up, long long left, long long diag, int32_t a, int32_t b, bool x_strip, int *dir) {
  const long long dc = diag + (a != b ? kKey64Sub : 0), uc = up + kKey64Edit, lc = left + kKey64Edit;
  long long v = uc < dc ? uc : dc;
  v = lc < v ? lc : v;
  const long long x_only = x_strip ? lc : uc;
  const int x_dir = x_strip ? kDirStrip : kDirStream;
  *dir = dc == v ? kDirPair : (x_only == v ? x_dir : kDirStrip + kDirStream - x_dir);
  return v;
}
// A lane's start in the block of tile k below row r0 (a multiple of 1024): the tokens of its columns, row r0 of them from the row
// checkpoint (r0 = 0: the closed form), and K[r0][its first column - 1] from the left neighbour's part of that checkpoint or, on lane 0,
// from the column checkpoint of tile k - 1 (tile 0: the closed form).  ld: how a checkpoint is read (the device reads past its caches).
template <class Ld> CTC_HD void align_lane_init(KeyLane64 &l, int lane, const int32_t *strip, int n, int k, int r0, const AlignSlot &s, Ld ld) {
  CountCell::init(l, lane, strip, n, k * kLongTile);
  if (r0 == 0) return;
  const long long *row = s.rowck + align_row_index(s, r0, k, lane * kLongC);
#pragma unroll
  for (int j = 0; j < kLongC; ++j) l.prev[j] = ld(row + j);
  l.diag = lane > 0 ? ld(row - 1) : (k > 0 ? ld(s.colck + align_col_index(s, k - 1, r0)) : CountCell::edge0(r0));
}
// lane 0's left edge of row r in tile k
template <class Ld> CTC_HD long long align_edge(const AlignSlot &s, int k, int r, Ld ld) {
  return k > 0 ? ld(s.colck + align_col_index(s, k - 1, r)) : CountCell::edge0(r);
}
// CountCell::step with directions, over the block's local rows 1 .. rows (s and lane_row count from the block's top).  -> did the lane
// compute a row at this step?  *word: the directions of its 32 cells.
CTC_HD bool align_lane_step(KeyLane64 &l, int lane, int s, int rows, long long in_left, int32_t in_tok, int32_t fresh, bool x_strip, uint64_t *word) {
  const int r = lane_row(s, lane);
  if (r < 1 || r > rows) return false;
  const int32_t t = lane == 0 ? fresh : in_tok;
  long long left = in_left, diag = l.diag;
  l.diag = left;
  l.tok = t;
  uint64_t w = 0;
#pragma unroll
  for (int k = 0; k < kLongC; ++k) {
    const long long up = l.prev[k];
    int dir;
    const long long v = key64_cell_dir(up, left, diag, l.a[k], t, x_strip, &dir);
    w |= (uint64_t)dir << (2 * k);
    diag = up;
    left = v;
    l.prev[k] = v;
  }
  *word = w;
  return true;
}
// the steps of a block's sweep that the walk needs: lane column lc finishes local row `rows` at step rows + lc - 1
CTC_HD int align_block_steps(int rows, int lc) { return rows + lc; }

// ---- one pair, sequentially (the host twin) ----------------------------------------------------------------------------------------------
// W simulated waves of 64 simulated lanes.  In a global block the waves run one after the other, the HIGHEST first: a consumer runs
// before its producer, so an edge that the schedule made it read in the block that completes it would be read stale.  ring: W rings
// of kLongRing values; col: the slot, long_slot_bytes of the call's dimensions.  -> D[m][n] or K[m][n].
// AlignCell: col is the slot's column checkpoints and ck the slot; the sweep keeps the checkpoints as the kernel does.
template <class P> inline typename P::V long_pair_host(const int32_t *strip, int n, const int32_t *stream, int m, int W, typename P::V *ring, typename P::V *col, typename P::L *lanes,
                                                       const AlignSlot *ck = nullptr) {
  typedef typename P::V V;
  const int tiles = long_tiles(n), steps = long_tile_steps(m), nb = long_tile_blocks(m);
  const long long G = long_blocks(m, n, W);
  V result = 0;
  for (long long g = 0; g < G; ++g)
    for (int w = W - 1; w >= 0; --w) {
      const LongSlot sl = long_slot(g, w, m, n, W);
      if (!sl.active) continue;
      typename P::L *L = lanes + (size_t)w * kEditLanes;
      const int k = sl.tile, s0 = sl.block * kLongBlock;
      if (sl.block == 0)
        for (int l = 0; l < kEditLanes; ++l) P::init(L[l], l, strip, n, k * kLongTile);
      V edge[kLongBlock];
      for (int i = 0; i < kLongBlock; ++i) {
        const int r = long_row_first(sl.block) + i;
        edge[i] = k == 0 || r > m ? P::edge0(r) : (w > 0 ? ring[(size_t)(w - 1) * kLongRing + long_ring_index(r)] : col[P::kCheckpoints ? align_col_index(*ck, k - 1, r) : (size_t)r]);
      }
      const bool to_ring = k + 1 < tiles && w + 1 < W, to_col = k + 1 < tiles && (P::kCheckpoints || w + 1 == W);
      const int cnt = steps - s0 < kLongBlock ? steps - s0 : kLongBlock;
      for (int q = 0; q < cnt; ++q) {
        const int s = s0 + q;
        V left[kEditLanes];
        int32_t tok[kEditLanes];
        for (int l = 0; l < kEditLanes; ++l) {
          left[l] = l > 0 ? P::last(L[l - 1]) : edge[q];
          tok[l] = l > 0 ? L[l - 1].tok : 0;
        }
        const int32_t fresh = s < m ? stream[s] : 0;
        for (int l = 0; l < kEditLanes; ++l) {
          P::step(L[l], l, s, m, left[l], tok[l], fresh);
          const int lr = lane_row(s, l);
          if (P::kCheckpoints && lr >= 1 && lr <= m && lr % kAlignBand == 0)
            for (int j = 0; j < kLongC; ++j) ck->rowck[align_row_index(*ck, lr, k, l * kLongC + j)] = L[l].prev[j];
        }
        const int r = long_edge_row(s);
        if (r >= 1 && r <= m) {
          if (to_ring) ring[(size_t)w * kLongRing + long_ring_index(r)] = P::last(L[kEditLanes - 1]);
          if (to_col) col[P::kCheckpoints ? align_col_index(*ck, k, r) : (size_t)r] = P::last(L[kEditLanes - 1]);
        }
      }
      if (k == tiles - 1 && sl.block == nb - 1) {
        const int nl = n - k * kLongTile;
        result = long_pick<P>(L[result_lane(nl, kLongC)], result_col(nl, kLongC));
      }
    }
  return result;
}

// ... and its alignment: the checkpointed sweep above, then the walk, block by block, through slot -- long_align_slot_bytes(L, Lq)
// bytes, m <= max(L, Lq), n <= min(L, Lq).  The maps hold -1 already.  -> K[m][n]; *blocks: the blocks the walk has swept again.
struct AlignHostLoad {
  long long operator()(const long long *p) const { return *p; }
};
inline void align_block_host(const int32_t *strip, int n, const int32_t *stream, int k, int r0, int rows, int lc, bool x_strip, const AlignSlot &s, KeyLane64 *L) {
  const AlignHostLoad ld;
  for (int l = 0; l < kEditLanes; ++l) align_lane_init(L[l], l, strip, n, k, r0, s, ld);
  const int steps = align_block_steps(rows, lc);
  for (int q = 0; q < steps; ++q) {
    long long left[kEditLanes];
    int32_t tok[kEditLanes];
    for (int l = 0; l < kEditLanes; ++l) {
      left[l] = l > 0 ? L[l - 1].prev[kLongC - 1] : (q < rows ? align_edge(s, k, r0 + q + 1, ld) : 0);
      tok[l] = l > 0 ? L[l - 1].tok : 0;
    }
    const int32_t fresh = q < rows ? stream[r0 + q] : 0;
    for (int l = 0; l < kEditLanes; ++l) {
      uint64_t w;
      if (align_lane_step(L[l], l, q, rows, left[l], tok[l], fresh, x_strip, &w) && l <= lc) s.dirs[align_dir_index(lane_row(q, l), l)] = w;
    }
  }
}
inline long long long_align_host(const int32_t *strip, int n, const int32_t *stream, int m, int W, bool x_strip, long long *ring, char *slot, int L, int Lq, KeyLane64 *lanes,
                                 int32_t *x_to_y, int32_t *y_to_x, int *blocks) {
  const AlignSlot s = align_slot(slot, L, Lq);
  const long long key = long_pair_host<AlignCell>(strip, n, stream, m, W, ring, s.colck, lanes, &s);
  int r = m, c = n;
  *blocks = 0;
  while (r > 0 && c > 0) {
    const int k = align_tile_of(c), r0 = align_row0_of(r), lo = k * kLongTile;
    align_block_host(strip, n, stream, k, r0, r - r0, (c - 1 - lo) / kLongC, x_strip, s, lanes);
    ++*blocks;
    while (r > r0 && c > lo) {
      const int dir = dir_of<kLongC>(s.dirs[align_dir_index(r - r0, (c - 1 - lo) / kLongC)], c);
      if (dir == kDirPair) walk_pair(r, c, x_strip, x_to_y, y_to_x);
      r -= walk_dr(dir), c -= walk_dc(dir);
    }
  }
  return key;
}

}  // namespace ctcedit

struct ctcd_decoder;
namespace ctcedit {
// what the long route needs of the library's host file: the waves ctcd_set_edit_long set (0: off), its two decoder-owned buffers -- the
// list of long pairs with its counter in front, and the slots -- and what ctcd_last_edit_long reads: whether the last call launched
// the long kernel, and on which stream
int edit_long_waves(const ctcd_decoder *d);
int edit_long_buffers(ctcd_decoder *d, size_t list_bytes, size_t slot_bytes, void **list, void **slots);
void edit_note_long(ctcd_decoder *d, bool launched, void *stream);

// editlong.hip: the plan of a call with the mode on and min(L, Lq) > 2048, and its two launches around the per-wave kernel's
struct LongPlan {
  unsigned *count;    // the number of long pairs, cleared by long_prepare, raised by the per-wave kernel <true>
  long long *list;    // their work indices
  char *slots;
  size_t slot_bytes;
  long long grid;     // workgroups = slots
  int waves;
};
int long_prepare(ctcd_decoder *d, const EditDecoderInfo &inf, const char *who, bool counts, int L, int Lq, long long work, void *stream, LongPlan *plan);
int long_launch(ctcd_decoder *d, const LongPlan &plan, bool counts, const int32_t *x, const int32_t *x_lens, int R, int L, const int32_t *y, const int32_t *y_lens, int Q,
                int Lq, int32_t *out, void *stream);
// ... and their align forms (ctcd_edit_align).  short_bytes: what the per-wave kernel's slots need; they and the long kernel's slots are
// used one after the other on the stream and share one allocation of the larger need, plan->slots.  The long kernel writes the maps
// and, counts != NULL, the counts of the listed pairs.
int long_prepare_align(ctcd_decoder *d, const EditDecoderInfo &inf, const char *who, int L, int Lq, long long work, size_t short_bytes, void *stream, LongPlan *plan);
int long_launch_align(ctcd_decoder *d, const LongPlan &plan, const int32_t *x, const int32_t *x_lens, int R, int L, const int32_t *y, const int32_t *y_lens, int Q, int Lq,
                      int32_t *x_to_y, int32_t *y_to_x, int32_t *counts, void *stream);
}  // namespace ctcedit
