// editlong.hip -- the long edit pairs of editlong.h on the device (include/ctcdecode_amd.h "Long edit pairs").  Three kernels:
//   edit_long_clear_kernel   one thread: the counter of the long-pair list to 0 (a kernel, so that the call can be captured in a graph).
//   edit_long_kernel<P>      a workgroup of W x 64 threads per long pair, a persistent grid that strides over the list the per-wave
//                            kernel <true> (editdist.hip, editops.hip) has left; the count is read from device memory.  Wave w sweeps
//                            tiles w, w + W, .. of the strip on editlong.h's schedule: the tile's tokens and its row of D (or of 64-bit
//                            keys) in registers, one-lane shifts inside the wave, the streamed row read 64 tokens a block ahead, the
//                            64 left edges of a block fetched at its top -- lane i holds row 64 j + 1 + i -- from the left neighbour's
//                            LDS ring or, for wave 0 beyond the first round, from the workgroup's slot, and handed to lane 0 by a read
//                            of one lane; lane 63 stores its last column after every row into the wave's ring or, on wave W - 1, into
//                            the slot.  A device-scope fence and a workgroup barrier end every block of 64 steps.
//   edit_long_align_kernel   ctcd_edit_align's long pairs: the CountCell sweep with checkpoints (AlignCell), then the walk on wave 0, block
//                            by block, each block swept again from its checkpoints with directions (editlong.h "Alignments").
// P: the cell policy, DistCell (one word) or CountCell (a 64-bit key).  Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "editlong.h"

namespace ctcedit {

__device__ __forceinline__ int long_shift_up(int v) { return __shfl_up(v, 1, kEditLanes); }
__device__ __forceinline__ long long long_shift_up(long long v) {
  const int lo = __shfl_up((int)(v & 0xffffffffll), 1, kEditLanes), hi = __shfl_up((int)(v >> 32), 1, kEditLanes);
  return ((long long)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ int long_read_lane(int v, int k) { return __builtin_amdgcn_readlane(v, k); }
__device__ __forceinline__ long long long_read_lane(long long v, int k) {
  const int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffll), k), hi = __builtin_amdgcn_readlane((int)(v >> 32), k);
  return ((long long)hi << 32) | (unsigned)lo;
}
// The slot's column.  It is written in one round and read in the next by another wave of the same workgroup; the loads and stores are
// relaxed device-scope atomics, so that none is served from a cache line an earlier round left behind.
template <class V> __device__ __forceinline__ V col_load(const V *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class V> __device__ __forceinline__ void col_store(V *p, V v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One pair on one workgroup: strip[0..n), stream[0..m), 1 <= n <= m.  ring: W rings of kLongRing values in LDS; col: the slot, m + 1
// values or more.  -> does this wave hold the result (it swept the last tile)?  *result: D[m][n] or K[m][n], in every lane of it.
// AlignCell: col is the slot's column checkpoints, a column per tile, and ck the slot; every wave stores its right edge there, and every
// lane its row at the multiples of kAlignBand.
template <class P>
__device__ __forceinline__ bool long_sweep(const int32_t *strip, int n, const int32_t *stream, int m, int lane, int wave, int W, typename P::V *ring,
                                           typename P::V *col, typename P::V *result, const AlignSlot *ck = nullptr) {
  typedef typename P::V V;
  typename P::L Ln;
  P::init(Ln, lane, strip, n, 0);
  const int tiles = long_tiles(n), steps = long_tile_steps(m);
  const long long G = long_blocks(m, n, W);
  int32_t nxt = 0;
  for (long long g = 0; g < G; ++g) {
    const LongSlot sl = long_slot(g, wave, m, n, W);  // (the same for the whole wave)
    if (sl.active) {
      const int k = sl.tile, j = sl.block, s0 = j * kLongBlock;
      if (j == 0) {
        P::init(Ln, lane, strip, n, k * kLongTile);
        nxt = lane < m ? stream[lane] : 0;
      }
      const int32_t cur = nxt;
      const int ahead = s0 + kLongBlock + lane;  // (< 2^30 + 128)
      nxt = ahead < m ? stream[ahead] : 0;
      // the block's left edges: lane i holds column 2048 k of row 64 j + 1 + i, complete since the barrier before this block
      const int er = long_row_first(j) + lane;
      V edge = P::edge0(er);
      if (k > 0 && er <= m) edge = wave > 0 ? ring[(wave - 1) * kLongRing + long_ring_index(er)] : col_load(col + (P::kCheckpoints ? align_col_index(*ck, k - 1, er) : (size_t)er));
      const bool to_ring = k + 1 < tiles && wave + 1 < W, to_col = k + 1 < tiles && (P::kCheckpoints || wave + 1 == W);
      const int cnt = steps - s0 < kLongBlock ? steps - s0 : kLongBlock;
      for (int q = 0; q < cnt; ++q) {
        const int s = s0 + q;
        const int32_t fresh = __builtin_amdgcn_readlane(cur, q);
        const V e = long_read_lane(edge, q);
        const V up = long_shift_up(P::last(Ln));
        const int32_t in_tok = long_shift_up(Ln.tok);
        P::step(Ln, lane, s, m, lane == 0 ? e : up, in_tok, fresh);
        const int r = long_edge_row(s);
        if (lane == kEditLanes - 1 && r >= 1 && r <= m) {  // (r <= m <= max(L, Lq): inside the slot)
          if (to_ring) ring[wave * kLongRing + long_ring_index(r)] = P::last(Ln);
          if (to_col) col_store(col + (P::kCheckpoints ? align_col_index(*ck, k, r) : (size_t)r), P::last(Ln));  // (k <= tiles - 2: inside the slot's columns)
        }
        // Plain stores suffice where the column has relaxed agent-scope ones: only this workgroup's wave 0 reads a row checkpoint, through
        // col_load past the L1 that all its waves share, behind the fence in front of a barrier -- and the L1 writes through.
        if (P::kCheckpoints) {  // the row checkpoint: 256 bytes per lane, once in 1024 steps (1024 <= row <= m: inside the slot's rows)
          const int lr = lane_row(s, lane);
          if (lr >= 1 && lr <= m && (lr & (kAlignBand - 1)) == 0) {
            long long *row = ck->rowck + align_row_index(*ck, lr, k, lane * kLongC);
#pragma unroll
            for (int c = 0; c < kLongC; ++c) row[c] = Ln.prev[c];
          }
        }
      }
    }
    __threadfence();  // the slot's column: stored before the barrier, loaded after it
    __syncthreads();
  }
  // the last tile is the last its wave has swept: the row of that tile is still in the wave's registers
  const int nl = n - (tiles - 1) * kLongTile;
  const V v = long_pick<P>(Ln, result_col(nl, kLongC));
  *result = long_read_lane(v, result_lane(nl, kLongC));
  return wave == (tiles - 1) % W;
}

__global__ void edit_long_clear_kernel(unsigned *count) { *count = 0u; }

template <class P>
__global__ void __launch_bounds__(kLongMaxWaves *kEditLanes) edit_long_kernel(const int32_t *x, const int32_t *x_lens, int R, int L, const int32_t *y, const int32_t *y_lens,
                                                                              int Q, int Lq, const long long *list, const unsigned *count, char *slots,
                                                                              size_t slot_bytes, int32_t *out) {
  typedef typename P::V V;
  __shared__ V ring[kLongMaxWaves * kLongRing];
  const bool pairwise = y == nullptr;  // (the host has set Q = R, Lq = L)
  const int lane = (int)threadIdx.x & (kEditLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kEditLanes), W = (int)blockDim.x / kEditLanes;
  V *col = (V *)(slots + (size_t)blockIdx.x * slot_bytes);
  const unsigned pairs = *count;
  for (unsigned q = blockIdx.x; q < pairs; q += gridDim.x) {
    const Pair p = pair_of(list[q], R, Q, pairwise);  // (a pair of a valid item with two non-empty rows: the per-wave kernel has looked)
    const int b = __builtin_amdgcn_readfirstlane(p.b), i = __builtin_amdgcn_readfirstlane(p.i), j = __builtin_amdgcn_readfirstlane(p.j);
    const size_t xi = (size_t)b * R + i, yj = pairwise ? (size_t)b * R + j : (size_t)b * Q + j;
    const int lx = __builtin_amdgcn_readfirstlane(x_lens[xi]), ly = __builtin_amdgcn_readfirstlane(pairwise ? x_lens[yj] : y_lens[yj]);
    const int32_t *xr = x + xi * (size_t)L, *yr = pairwise ? x + yj * (size_t)L : y + yj * (size_t)Lq;
    const bool x_strip = lx <= ly;
    const int32_t *strip = x_strip ? xr : yr, *stream = x_strip ? yr : xr;
    const int n = x_strip ? lx : ly, m = x_strip ? ly : lx;
    V v;
    if (long_sweep<P>(strip, n, stream, m, lane, wave, W, ring, col, &v) && lane == 0)
      P::result(v, lx, ly, out + (((size_t)b * R + i) * Q + j) * P::kOutWords, pairwise ? out + (((size_t)b * R + j) * Q + i) * P::kOutWords : nullptr);
  }
}

// ---- alignments ----------------------------------------------------------------------------------------------------------------------
// a checkpoint is read by another wave than the one that stored it, a pair or a round later: past the caches, like the slot's column
struct AlignDeviceLoad {
  __device__ __forceinline__ long long operator()(const long long *p) const { return col_load(p); }
};
// The block of tile k below row r0 again, on one wave, up to local row `rows` and lane column lc: long_sweep's step with directions.
// The streamed tokens r0 .. r0 + rows - 1 are read 64 ahead, the 64 left edges of 64 steps at once; the direction words of local row
// 1 .. rows <= 1024 and lane <= lc go to the slot's block buffer (1024 x 64 words).
__device__ __forceinline__ void long_block_sweep(const int32_t *strip, int n, const int32_t *stream, int k, int r0, int rows, int lc, int lane, bool x_strip, const AlignSlot &ck) {
  const AlignDeviceLoad ld;
  KeyLane64 Ln;
  align_lane_init(Ln, lane, strip, n, k, r0, ck, ld);
  const int steps = align_block_steps(rows, lc);
  int32_t nxt = lane < rows ? stream[r0 + lane] : 0;
  for (int s0 = 0; s0 < steps; s0 += kLongBlock) {
    const int32_t cur = nxt;
    const int ahead = s0 + kLongBlock + lane;
    nxt = ahead < rows ? stream[r0 + ahead] : 0;
    const int er = s0 + 1 + lane;  // the local row whose left edge this lane fetches
    const long long edge = er <= rows ? align_edge(ck, k, r0 + er, ld) : 0;
    const int cnt = steps - s0 < kLongBlock ? steps - s0 : kLongBlock;
    for (int q = 0; q < cnt; ++q) {
      const int32_t fresh = __builtin_amdgcn_readlane(cur, q);
      const long long e = long_read_lane(edge, q);
      const long long up = long_shift_up(Ln.prev[kLongC - 1]);
      const int32_t in_tok = long_shift_up(Ln.tok);
      uint64_t w;
      const bool did = align_lane_step(Ln, lane, s0 + q, rows, lane == 0 ? e : up, in_tok, fresh, x_strip, &w);
      if (did && lane <= lc) ck.dirs[align_dir_index(lane_row(s0 + q, lane), lane)] = w;
    }
  }
}
// The canonical walk back from (m, n), block by block, on one wave; r and c are the same in every lane.  Inside a block it is
// editops.hip's walk: lane t loads the word of row rtop - t in the lane column of c, and the walk reads the direction of its row from
// that lane until it leaves the lane column, the 64 rows or the block.
__device__ __forceinline__ void long_walk(const int32_t *strip, int n, const int32_t *stream, int m, int lane, bool x_strip, const AlignSlot &ck, int32_t *x_to_y, int32_t *y_to_x) {
  int r = m, c = n;
  while (r > 0 && c > 0) {
    const int k = align_tile_of(c), r0 = align_row0_of(r), lo = k * kLongTile;
    long_block_sweep(strip, n, stream, k, r0, r - r0, (c - 1 - lo) / kLongC, lane, x_strip, ck);
    // The words were stored by other lanes than the ones that load them, but by this wave: its plain stores and loads go through one
    // L1 in order, so the fence only has to wait for the stores (no other wave touches the block buffer: the kernel's barrier).
    __threadfence();
    while (r > r0 && c > lo) {
      const int rtop = r, lc = (c - 1 - lo) / kLongC, clo = lo + lc * kLongC;
      const int row = rtop - lane;
      const uint64_t w = row > r0 ? ck.dirs[align_dir_index(row - r0, lc)] : 0;
      while (r > r0 && c > clo && rtop - r < kEditLanes) {
        const int dir = __builtin_amdgcn_readlane(dir_of<kLongC>(w, c), rtop - r);
        if (dir == kDirPair && lane == 0) walk_pair(r, c, x_strip, x_to_y, y_to_x);
        r -= walk_dr(dir), c -= walk_dc(dir);
      }
    }
  }
}

// General mode only.  The maps of every listed pair hold -1 (the per-wave kernel <true> has filled them); the sweep's last wave writes
// the counts, wave 0 walks, and a barrier keeps the other waves off the slot until it has.
__global__ void __launch_bounds__(kLongMaxWaves *kEditLanes) edit_long_align_kernel(const int32_t *x, const int32_t *x_lens, int R, int L, const int32_t *y, const int32_t *y_lens,
                                                                                    int Q, int Lq, const long long *list, const unsigned *count, char *slots,
                                                                                    size_t slot_bytes, int32_t *x_to_y, int32_t *y_to_x, int32_t *counts) {
  __shared__ long long ring[kLongMaxWaves * kLongRing];
  const int lane = (int)threadIdx.x & (kEditLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kEditLanes), W = (int)blockDim.x / kEditLanes;
  const AlignSlot ck = align_slot(slots + (size_t)blockIdx.x * slot_bytes, L, Lq);
  const unsigned pairs = *count;
  for (unsigned q = blockIdx.x; q < pairs; q += gridDim.x) {
    const long long w = list[q];  // (the pair's row-major index: where its maps and counts are)
    const Pair p = pair_of(w, R, Q, false);
    const int b = __builtin_amdgcn_readfirstlane(p.b), i = __builtin_amdgcn_readfirstlane(p.i), j = __builtin_amdgcn_readfirstlane(p.j);
    const size_t xi = (size_t)b * R + i, yj = (size_t)b * Q + j;
    const int lx = __builtin_amdgcn_readfirstlane(x_lens[xi]), ly = __builtin_amdgcn_readfirstlane(y_lens[yj]);
    const int32_t *xr = x + xi * (size_t)L, *yr = y + yj * (size_t)Lq;
    const bool x_strip = lx <= ly;
    const int32_t *strip = x_strip ? xr : yr, *stream = x_strip ? yr : xr;
    const int n = x_strip ? lx : ly, m = x_strip ? ly : lx;  // n <= min(L, Lq), m <= max(L, Lq): inside the slot's parts
    long long v;
    if (long_sweep<AlignCell>(strip, n, stream, m, lane, wave, W, ring, ck.colck, &v, &ck) && lane == 0 && counts) CountCell::result(v, lx, ly, counts + (size_t)w * 4, nullptr);
    // (the sweep has ended with a fence and a barrier: the checkpoints are complete)
    if (wave == 0) long_walk(strip, n, stream, m, lane, x_strip, ck, x_to_y + (size_t)w * L, y_to_x + (size_t)w * Lq);
    __syncthreads();
  }
}

int long_prepare(ctcd_decoder *d, const EditDecoderInfo &inf, const char *who, bool counts, int L, int Lq, long long work, void *stream, LongPlan *plan) {
  const std::string f = who;
  plan->waves = edit_long_waves(d);
  plan->slot_bytes = long_slot_bytes(L, Lq, counts);
  // a workgroup per slot: ctcd_set_edit_grid's cap (at most 2^20), or one per compute unit; never more than there are pairs
  const long long cap = inf.cap > 0 ? (inf.cap < (1ll << 20) ? inf.cap : (1ll << 20)) : (long long)(inf.cus > 0 ? inf.cus : 1);
  const long long budget = edit_budget(d) > 0 ? edit_budget(d) : kOpsDefaultScratch, fit = budget / (long long)plan->slot_bytes;
  if (fit < 1)
    return edit_fail(CTCD_EUNSUPPORTED, (f + "one slot of " + std::to_string(plan->slot_bytes) + " bytes (max(L, Lq) + 1 edges of a long pair) does not fit the scratch budget of " +
                                         std::to_string(budget) + " bytes (ctcd_set_edit_scratch)").c_str());
  long long grid = cap < work ? cap : work;
  grid = grid < fit ? grid : fit;
  plan->grid = grid < 1 ? 1 : grid;
  void *list = nullptr, *slots = nullptr;
  // the counter and a word of padding in front of the list
  if (const int rc = edit_long_buffers(d, 8 + (size_t)work * 8, (size_t)plan->grid * plan->slot_bytes, &list, &slots)) return rc;
  plan->count = (unsigned *)list;
  plan->list = (long long *)((char *)list + 8);
  plan->slots = (char *)slots;
  hipLaunchKernelGGL(edit_long_clear_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, plan->count);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return edit_fail(CTCD_EHIP, (f + hipGetErrorString(e)).c_str());
  return CTCD_OK;
}

int long_launch(ctcd_decoder *d, const LongPlan &plan, bool counts, const int32_t *x, const int32_t *x_lens, int R, int L, const int32_t *y, const int32_t *y_lens, int Q,
                int Lq, int32_t *out, void *stream) {
  const dim3 grid((unsigned)plan.grid), block((unsigned)(plan.waves * kEditLanes));
  if (counts)
    hipLaunchKernelGGL(edit_long_kernel<CountCell>, grid, block, 0, (hipStream_t)stream, x, x_lens, R, L, y, y_lens, Q, Lq, (const long long *)plan.list,
                       (const unsigned *)plan.count, plan.slots, plan.slot_bytes, out);
  else
    hipLaunchKernelGGL(edit_long_kernel<DistCell>, grid, block, 0, (hipStream_t)stream, x, x_lens, R, L, y, y_lens, Q, Lq, (const long long *)plan.list,
                       (const unsigned *)plan.count, plan.slots, plan.slot_bytes, out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return edit_fail(CTCD_EHIP, (std::string("long edit pairs: ") + hipGetErrorString(e)).c_str());
  edit_note_long(d, true, stream);
  edit_note_slots(d, plan.grid);
  return CTCD_OK;
}

int long_prepare_align(ctcd_decoder *d, const EditDecoderInfo &inf, const char *who, int L, int Lq, long long work, size_t short_bytes, void *stream, LongPlan *plan) {
  const std::string f = who;
  plan->waves = edit_long_waves(d);
  plan->slot_bytes = long_align_slot_bytes(L, Lq);
  const long long cap = inf.cap > 0 ? (inf.cap < (1ll << 20) ? inf.cap : (1ll << 20)) : (long long)(inf.cus > 0 ? inf.cus : 1);
  const long long budget = edit_budget(d) > 0 ? edit_budget(d) : kOpsDefaultScratch, fit = budget / (long long)plan->slot_bytes;
  if (fit < 1)
    return edit_fail(CTCD_EUNSUPPORTED, (f + "one slot of " + std::to_string(plan->slot_bytes) + " bytes (the checkpoints and the block buffer of a long pair) does not fit the scratch budget of " +
                                         std::to_string(budget) + " bytes (ctcd_set_edit_scratch)").c_str());
  long long grid = cap < work ? cap : work;
  grid = grid < fit ? grid : fit;
  plan->grid = grid < 1 ? 1 : grid;
  void *list = nullptr, *unused = nullptr, *slots = nullptr;
  const size_t long_bytes = (size_t)plan->grid * plan->slot_bytes;
  if (const int rc = edit_long_buffers(d, 8 + (size_t)work * 8, 0, &list, &unused)) return rc;
  if (const int rc = edit_scratch(d, short_bytes > long_bytes ? short_bytes : long_bytes, &slots)) return rc;
  plan->count = (unsigned *)list;
  plan->list = (long long *)((char *)list + 8);
  plan->slots = (char *)slots;
  hipLaunchKernelGGL(edit_long_clear_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, plan->count);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return edit_fail(CTCD_EHIP, (f + hipGetErrorString(e)).c_str());
  return CTCD_OK;
}

int long_launch_align(ctcd_decoder *d, const LongPlan &plan, const int32_t *x, const int32_t *x_lens, int R, int L, const int32_t *y, const int32_t *y_lens, int Q, int Lq,
                      int32_t *x_to_y, int32_t *y_to_x, int32_t *counts, void *stream) {
  hipLaunchKernelGGL(edit_long_align_kernel, dim3((unsigned)plan.grid), dim3((unsigned)(plan.waves * kEditLanes)), 0, (hipStream_t)stream, x, x_lens, R, L, y, y_lens, Q, Lq,
                     (const long long *)plan.list, (const unsigned *)plan.count, plan.slots, plan.slot_bytes, x_to_y, y_to_x, counts);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return edit_fail(CTCD_EHIP, (std::string("long edit alignments: ") + hipGetErrorString(e)).c_str());
  edit_note_long(d, true, stream);
  edit_note_slots(d, plan.grid);
  return CTCD_OK;
}

}  // namespace ctcedit
