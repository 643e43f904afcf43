// editlong.hip -- the long edit pairs of editlong.h on the device (include/ctcdecode_amd.h "Long edit pairs").  Two kernels:
//   edit_long_clear_kernel   one thread: the counter of the long-pair list to 0 (a kernel, so that the call can be captured in a graph).
//   edit_long_kernel<P>      a workgroup of W x 64 threads per long pair, a persistent grid that strides over the list the per-wave
//                            kernel <true> (editdist.hip, editops.hip) has left; the count is read from device memory.  Wave w sweeps
//                            tiles w, w + W, .. of the strip on editlong.h's schedule: the tile's tokens and its row of D (or of 64-bit
//                            keys) in registers, one-lane shifts inside the wave, the streamed row read 64 tokens a block ahead, the
//                            64 left edges of a block fetched at its top -- lane i holds row 64 j + 1 + i -- from the left neighbour's
//                            LDS ring or, for wave 0 beyond the first round, from the workgroup's slot, and handed to lane 0 by a read
//                            of one lane; lane 63 stores its last column after every row into the wave's ring or, on wave W - 1, into
//                            the slot.  A device-scope fence and a workgroup barrier end every block of 64 steps.
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
template <class P>
__device__ __forceinline__ bool long_sweep(const int32_t *strip, int n, const int32_t *stream, int m, int lane, int wave, int W, typename P::V *ring,
                                           typename P::V *col, typename P::V *result) {
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
      if (k > 0 && er <= m) edge = wave > 0 ? ring[(wave - 1) * kLongRing + long_ring_index(er)] : col_load(col + er);
      const bool to_ring = k + 1 < tiles && wave + 1 < W, to_col = k + 1 < tiles && wave + 1 == W;
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
          if (to_col) col_store(col + r, P::last(Ln));
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

}  // namespace ctcedit
