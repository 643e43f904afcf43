// editdist.hip -- the Levenshtein distances of editdist.h on the device, and their C ABI (include/ctcdecode_amd.h "Edit distance").
// A translation unit of its own, like greedy.hip: no kernel of another file sees it.  One kernel:
//   edit_distance_kernel   a wave per pair, four pairs per workgroup, a persistent grid that strides over the work index of
//                          editdist.h pair_of.  The wave reads the pair's two lengths, takes the shorter row as the strip, and
//                          branches -- uniformly -- into the sweep of the strip's class (C = 1 .. 32 columns per lane).  The strip's
//                          tokens and the lane's row of D stay in registers; a lane's last column and its streamed token move to the
//                          next lane by a one-lane shift across the wave; the streamed row is read 64 tokens at a time, a block
//                          ahead of its use, and handed to lane 0 by a read of one lane.  No LDS, no scratch.
// Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "editdist.h"

namespace ctcedit {

// The one-lane shift.  __shfl_up is one ds_bpermute_b32: it goes through the LDS crossbar, not through LDS memory, and reaches across
// all 64 lanes -- the DPP row shifts stop at rows of 16 lanes, and stitching the rows together would add instructions to a step that
// is bound by instruction issue more than by the shifts' latency.  Lane 0 receives its own value and does not look at it.
__device__ __forceinline__ int shift_up(int v) { return __shfl_up(v, 1, kEditLanes); }

// The sweep of one pair on one wave: strip[0..n), 1 <= n <= 64 * C; stream[0..m), m >= n.  -> D[m][n], in every lane.
template <int C> __device__ __forceinline__ int sweep(const int32_t *strip, int n, const int32_t *stream, int m, int lane) {
  Lane<C> L;
  lane_init(L, lane, strip, n);
  const int steps = sweep_steps(m, n, C);
  // the streamed row, 64 tokens at a time: lane j of `cur` holds stream[s0 + j]; the block after it is on its way while this one is
  // used (the copy at the top of a block is the only place that waits for a load, and that load is a block old)
  int32_t nxt = lane < m ? stream[lane] : 0;
  for (int s0 = 0; s0 < steps; s0 += kEditLanes) {
    const int32_t cur = nxt;
    const int ahead = s0 + kEditLanes + lane;  // (< 2^30 + 128)
    nxt = ahead < m ? stream[ahead] : 0;
    const int cnt = steps - s0 < kEditLanes ? steps - s0 : kEditLanes;
    for (int k = 0; k < cnt; ++k) {
      const int32_t fresh = __builtin_amdgcn_readlane(cur, k);
      const int in_left = shift_up(L.prev[C - 1]);
      const int32_t in_tok = shift_up(L.tok);
      lane_step(L, lane, s0 + k, m, in_left, in_tok, fresh);
    }
  }
  // (a select chain, not an indexed read: the row stays in registers)
  const int col = result_col(n, C);
  int v = L.prev[0];
#pragma unroll
  for (int k = 1; k < C; ++k) v = k == col ? L.prev[k] : v;
  return __shfl(v, result_lane(n, C), kEditLanes);
}

// are all lengths of item b inside their bounds?  (the wave reads them side by side; y_lens == NULL: pairwise mode)
__device__ __forceinline__ bool item_ok_wave(const int32_t *x_lens, int b, int R, int L, const int32_t *y_lens, int Q, int Lq, int lane) {
  bool ok = true;
  for (int i = lane; i < R; i += kEditLanes) ok = ok && len_ok(x_lens[(size_t)b * R + i], L);
  if (y_lens)
    for (int j = lane; j < Q; j += kEditLanes) ok = ok && len_ok(y_lens[(size_t)b * Q + j], Lq);
  return __ballot(!ok) == 0ull;
}

__global__ void __launch_bounds__(kEditThreads) edit_distance_kernel(const int32_t *x, const int32_t *x_lens, int B, int R, int L, const int32_t *y,
                                                                    const int32_t *y_lens, int Q, int Lq, long long work, int32_t *out, int32_t *status) {
  const bool pairwise = y == nullptr;  // (the host has set Q = R, Lq = L)
  const int lane = (int)threadIdx.x & (kEditLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kEditLanes);
  const long long stride = (long long)gridDim.x * kEditWaves;
  int checked = -1;
  bool ok = true;
  for (long long w = (long long)blockIdx.x * kEditWaves + wave; w < work; w += stride) {
    const Pair p = pair_of(w, R, Q, pairwise);
    const int b = __builtin_amdgcn_readfirstlane(p.b), i = __builtin_amdgcn_readfirstlane(p.i), j = __builtin_amdgcn_readfirstlane(p.j);
    if (b != checked) {
      ok = item_ok_wave(x_lens, b, R, L, pairwise ? nullptr : y_lens, Q, Lq, lane);
      checked = b;
      if (!ok && status && lane == 0) status[b] = EDIT_BAD_ROW;  // (raised only)
    }
    int d = 0;
    if (ok) {
      const size_t xi = (size_t)b * R + i, yj = pairwise ? (size_t)b * R + j : (size_t)b * Q + j;
      const int lx = __builtin_amdgcn_readfirstlane(x_lens[xi]), ly = __builtin_amdgcn_readfirstlane(pairwise ? x_lens[yj] : y_lens[yj]);
      if (!pair_trivial(lx, ly, &d)) {
        const int32_t *xr = x + xi * (size_t)L, *yr = pairwise ? x + yj * (size_t)L : y + yj * (size_t)Lq;
        const bool x_strip = lx <= ly;
        const int32_t *strip = x_strip ? xr : yr, *stream = x_strip ? yr : xr;
        const int n = x_strip ? lx : ly, m = x_strip ? ly : lx;  // 1 <= n <= min(L, Lq) <= 2048, n <= m
        switch (strip_class(n)) {  // (the same for the whole wave)
          case 1: d = sweep<1>(strip, n, stream, m, lane); break;
          case 2: d = sweep<2>(strip, n, stream, m, lane); break;
          case 4: d = sweep<4>(strip, n, stream, m, lane); break;
          case 8: d = sweep<8>(strip, n, stream, m, lane); break;
          case 16: d = sweep<16>(strip, n, stream, m, lane); break;
          default: d = sweep<32>(strip, n, stream, m, lane);
        }
      }
    }
    if (lane == 0) {
      out[((size_t)b * R + i) * Q + j] = d;
      if (pairwise) out[((size_t)b * R + j) * Q + i] = d;
    }
  }
  if (pairwise) {  // the diagonal; a row's own length is looked at here, so that an item of one row is validated too
    const long long rows = (long long)B * R;
    for (long long k = (long long)blockIdx.x * kEditThreads + threadIdx.x; k < rows; k += (long long)gridDim.x * kEditThreads) {
      const long long b = k / R, i = k - b * R;
      out[((size_t)b * R + i) * R + i] = 0;
      if (status && !len_ok(x_lens[k], L)) status[b] = EDIT_BAD_ROW;
    }
  }
}

}  // namespace ctcedit

using namespace ctcedit;

extern "C" {

int ctcd_edit_distance(ctcd_decoder *d, const int32_t *x, const int32_t *x_lens, int B, int R, int L, const int32_t *y, const int32_t *y_lens, int Q, int Lq,
                       int32_t *out, int32_t *status, void *stream) {
  const std::string f = "ctcd_edit_distance: ";
  if (!d) return edit_fail(CTCD_EINVAL, "decoder == NULL");
  const bool pairwise = y == nullptr;
  if (pairwise) Q = R, Lq = L;
  if (B < 0 || R < 0 || L < 0 || Q < 0 || Lq < 0) return edit_fail(CTCD_EINVAL, (f + "B, R, L, Q, Lq >= 0 required").c_str());
  EditDecoderInfo inf;
  if (const int rc = edit_decoder_info(d, &inf)) return rc;
  if (B == 0 || R == 0 || Q == 0) {
    edit_note_pairs(d, 0, 0);
    return CTCD_OK;
  }
  if (!x_lens || !out || (!x && L > 0) || (!pairwise && !y_lens)) return edit_fail(CTCD_EINVAL, (f + "null tensor").c_str());
  if ((L < Lq ? L : Lq) > kEditMaxStrip)
    return edit_fail(CTCD_EUNSUPPORTED, (f + "min(L, Lq) > 2048: the shorter row of a pair lives in one wave's registers, 32 columns per lane").c_str());
  if (L > kEditMaxDim || Lq > kEditMaxDim) return edit_fail(CTCD_EUNSUPPORTED, (f + "rows of more than 2^30 positions").c_str());
  if ((long long)B * R > 0x7fffffffLL || (long long)B * Q > 0x7fffffffLL) return edit_fail(CTCD_EUNSUPPORTED, (f + "too many rows for one launch").c_str());
  const long long work = pairs_per_item(R, Q, pairwise) * B;
  ctcdev::DeviceGuard guard;
  if (guard.enter(inf.device) != hipSuccess) return edit_fail(CTCD_EHIP, (std::string("hipSetDevice: ") + hipGetErrorString(guard.err)).c_str());
  // ctcd_set_edit_grid's cap (at most 2^20 workgroups), or two workgroups per compute unit
  const long long cap = inf.cap > 0 ? (inf.cap < (1ll << 20) ? inf.cap : (1ll << 20)) : (long long)(inf.cus > 0 ? inf.cus : 1) * (kEditWavesPerCu / kEditWaves);
  long long grid = (work + kEditWaves - 1) / kEditWaves;
  grid = grid < 1 ? 1 : (grid > cap ? cap : grid);  // (a pairwise call of one-row items has no pair and a diagonal to write)
  hipLaunchKernelGGL(edit_distance_kernel, dim3((unsigned)grid), dim3(kEditThreads), 0, (hipStream_t)stream, x, x_lens, B, R, L, y, y_lens, Q, Lq, work, out,
                     status);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return edit_fail(CTCD_EHIP, (std::string("edit distance: ") + hipGetErrorString(e)).c_str());
  edit_note_pairs(d, work, grid);
  return CTCD_OK;
}

}  // extern "C"
