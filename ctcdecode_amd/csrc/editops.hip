// editops.hip -- edit-operation counts and token alignments on the device (editops.h; include/ctcdecode_amd.h "Edit operations"), and
// their C ABI.  A translation unit of its own beside editdist.hip, whose kernel it leaves alone.  Two kernels, both on editdist.hip's
// schedule -- a wave per pair, four pairs per workgroup, a persistent grid, the shorter row as the strip in registers, the longer one
// streamed past it 64 tokens ahead, two one-lane shifts per step -- over the packed key (D, S) of editops.h:
//   edit_counts_kernel   the sweep and an epilogue that turns K[m][n] and the two lengths into (H, S, Del, I).  No LDS, no scratch.
//   edit_align_kernel    the sweep also resolves, per cell, the direction the canonical walk takes there, in x / y terms from the
//                        wave-uniform role flag; a lane's C directions of a step are one 32- or 64-bit word, stored to the wave's slot
//                        of the decoder-owned back-pointer scratch.  Then the wave walks back from (lx, ly): it fetches 64 rows of the
//                        lane column the walk stands in at once, a row per lane, and steps through them in registers until the walk
//                        leaves the column or the rows.
// Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "editops.h"

namespace ctcedit {

// the one-lane shift of editdist.hip (one ds_bpermute_b32 across all 64 lanes; lane 0 does not look at what it receives)
__device__ __forceinline__ int ops_shift_up(int v) { return __shfl_up(v, 1, kEditLanes); }

// The sweep of one pair on one wave over keys: strip[0..n), 1 <= n <= 64 * C; stream[0..m), m >= n.  -> K[m][n], in every lane.
// DIRS: the lanes up to the result's store their directions of row r to slot[r - 1][lane], r = 1 .. m.
template <int C, bool DIRS>
__device__ __forceinline__ int key_sweep(const int32_t *strip, int n, const int32_t *stream, int m, int lane, bool x_strip, typename DirWord<C>::type *slot) {
  Lane<C> L;
  key_lane_init(L, lane, strip, n);
  const int steps = sweep_steps(m, n, C), last = result_lane(n, C);
  int32_t nxt = lane < m ? stream[lane] : 0;
  for (int s0 = 0; s0 < steps; s0 += kEditLanes) {
    const int32_t cur = nxt;
    const int ahead = s0 + kEditLanes + lane;
    nxt = ahead < m ? stream[ahead] : 0;
    const int cnt = steps - s0 < kEditLanes ? steps - s0 : kEditLanes;
    for (int k = 0; k < cnt; ++k) {
      const int32_t fresh = __builtin_amdgcn_readlane(cur, k);
      const int in_left = ops_shift_up(L.prev[C - 1]);
      const int32_t in_tok = ops_shift_up(L.tok);
      typename DirWord<C>::type w;
      const bool did = key_lane_step<C, DIRS>(L, lane, s0 + k, m, in_left, in_tok, fresh, x_strip, &w);
      if (DIRS && did && lane <= last) slot[slot_index(lane_row(s0 + k, lane), lane)] = w;  // (1 <= row <= m: inside the slot)
    }
  }
  const int col = result_col(n, C);
  int v = L.prev[0];
#pragma unroll
  for (int k = 1; k < C; ++k) v = k == col ? L.prev[k] : v;
  return __shfl(v, last, kEditLanes);
}

// The canonical walk back from (m, n) over the slot the sweep has filled.  r and c are the same in every lane.  A block: lane t loads
// the word of row r0 - t in the lane column of c; the walk reads the direction of its row from that lane until it leaves the column
// or the 64 rows (a diagonal run crosses a column of C cells in C steps, a run of stream-only steps uses all 64 rows).
template <int C>
__device__ __forceinline__ void walk(const typename DirWord<C>::type *slot, int n, int m, bool x_strip, int32_t *x_to_y, int32_t *y_to_x, int lane) {
  int r = m, c = n;
  while (r > 0 && c > 0) {
    const int r0 = r, lc = (c - 1) / C, lo = lc * C;  // the column's cells: lo + 1 .. lo + C
    const int row = r0 - lane;
    const typename DirWord<C>::type w = row >= 1 ? slot[slot_index(row, lc)] : 0;
    while (r > 0 && c > lo && r0 - r < kEditLanes) {
      const int dir = __builtin_amdgcn_readlane(dir_of<C>(w, c), r0 - r);
      if (dir == kDirPair && lane == 0) walk_pair(r, c, x_strip, x_to_y, y_to_x);
      r -= walk_dr(dir), c -= walk_dc(dir);
    }
  }
}

template <int C>
__device__ __forceinline__ int align_class(const int32_t *strip, int n, const int32_t *stream, int m, int lane, bool x_strip, void *slot, int32_t *x_to_y, int32_t *y_to_x) {
  typedef typename DirWord<C>::type W;
  const int key = key_sweep<C, true>(strip, n, stream, m, lane, x_strip, (W *)slot);
  // the directions, and the -1 the wave has written over the maps, were stored by other lanes than the one that reads or overwrites them
  __threadfence();
  walk<C>((const W *)slot, n, m, x_strip, x_to_y, y_to_x, lane);
  return key;
}

// are all lengths of item b inside their bounds?  (the wave reads them side by side; y_lens == NULL: pairwise mode)
__device__ __forceinline__ bool ops_item_ok(const int32_t *x_lens, int b, int R, int L, const int32_t *y_lens, int Q, int Lq, int lane) {
  bool ok = true;
  for (int i = lane; i < R; i += kEditLanes) ok = ok && len_ok(x_lens[(size_t)b * R + i], L);
  if (y_lens)
    for (int j = lane; j < Q; j += kEditLanes) ok = ok && len_ok(y_lens[(size_t)b * Q + j], Lq);
  return __ballot(!ok) == 0ull;
}

__global__ void __launch_bounds__(kEditThreads) edit_counts_kernel(const int32_t *x, const int32_t *x_lens, int B, int R, int L, const int32_t *y,
                                                                  const int32_t *y_lens, int Q, int Lq, long long work, int32_t *out, int32_t *status) {
  const bool pairwise = y == nullptr;  // (the host has set Q = R, Lq = L)
  const int lane = (int)threadIdx.x & (kEditLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kEditLanes);
  const long long stride = (long long)gridDim.x * kEditWaves, first = (long long)blockIdx.x * kEditWaves + wave;
  int checked = -1;
  bool ok = true;
  for (long long w = first; w < work; w += stride) {
    const Pair p = pair_of(w, R, Q, pairwise);
    const int b = __builtin_amdgcn_readfirstlane(p.b), i = __builtin_amdgcn_readfirstlane(p.i), j = __builtin_amdgcn_readfirstlane(p.j);
    if (b != checked) {
      ok = ops_item_ok(x_lens, b, R, L, pairwise ? nullptr : y_lens, Q, Lq, lane);
      checked = b;
      if (!ok && status && lane == 0) status[b] = EDIT_BAD_ROW;  // (raised only)
    }
    int32_t cnt[4] = {0, 0, 0, 0};
    if (ok) {
      const size_t xi = (size_t)b * R + i, yj = pairwise ? (size_t)b * R + j : (size_t)b * Q + j;
      const int lx = __builtin_amdgcn_readfirstlane(x_lens[xi]), ly = __builtin_amdgcn_readfirstlane(pairwise ? x_lens[yj] : y_lens[yj]);
      int key = key_trivial(lx, ly);
      if (lx != 0 && ly != 0) {
        const int32_t *xr = x + xi * (size_t)L, *yr = pairwise ? x + yj * (size_t)L : y + yj * (size_t)Lq;
        const bool x_strip = lx <= ly;
        const int32_t *strip = x_strip ? xr : yr, *stream = x_strip ? yr : xr;
        const int n = x_strip ? lx : ly, m = x_strip ? ly : lx;  // 1 <= n <= min(L, Lq) <= 2048, n <= m <= 2^18
        switch (strip_class(n)) {  // (the same for the whole wave)
          case 1: key = key_sweep<1, false>(strip, n, stream, m, lane, x_strip, nullptr); break;
          case 2: key = key_sweep<2, false>(strip, n, stream, m, lane, x_strip, nullptr); break;
          case 4: key = key_sweep<4, false>(strip, n, stream, m, lane, x_strip, nullptr); break;
          case 8: key = key_sweep<8, false>(strip, n, stream, m, lane, x_strip, nullptr); break;
          case 16: key = key_sweep<16, false>(strip, n, stream, m, lane, x_strip, nullptr); break;
          default: key = key_sweep<32, false>(strip, n, stream, m, lane, x_strip, nullptr);
        }
      }
      counts_of(key, lx, ly, cnt);  // in x / y terms: a streamed x has its Del and I the right way round
    }
    if (lane == 0) {
      int32_t *o = out + (((size_t)b * R + i) * Q + j) * 4;
      o[0] = cnt[0], o[1] = cnt[1], o[2] = cnt[2], o[3] = cnt[3];
      if (pairwise) {  // row j as x: what it inserts is what row i deletes
        int32_t *t = out + (((size_t)b * R + j) * Q + i) * 4;
        t[0] = cnt[0], t[1] = cnt[1], t[2] = cnt[3], t[3] = cnt[2];
      }
    }
  }
  if (pairwise) {  // the diagonal, an item per wave: (len, 0, 0, 0), and zeros for an invalid item -- an item of one row is validated here
    for (long long b = first; b < B; b += stride) {
      const bool good = ops_item_ok(x_lens, (int)b, R, L, nullptr, Q, Lq, lane);
      if (!good && status && lane == 0) status[b] = EDIT_BAD_ROW;
      for (int i = lane; i < R; i += kEditLanes) {
        int32_t *o = out + (((size_t)b * R + i) * R + i) * 4;
        o[0] = good ? x_lens[(size_t)b * R + i] : 0;
        o[1] = o[2] = o[3] = 0;
      }
    }
  }
}

// General mode only.  slots: the waves that have a slot of slot_bytes in scratch, wave g the g-th; the others leave at once, and the
// waves that stay stride over the pairs by their own number.
__global__ void __launch_bounds__(kEditThreads) __attribute__((amdgpu_waves_per_eu(2))) edit_align_kernel(const int32_t *x, const int32_t *x_lens, int R, int L, const int32_t *y, const int32_t *y_lens,
                                                                 int Q, int Lq, long long work, char *scratch, size_t slot_bytes, long long slots,
                                                                 int32_t *x_to_y, int32_t *y_to_x, int32_t *counts, int32_t *status) {
  const int lane = (int)threadIdx.x & (kEditLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kEditLanes);
  const long long first = (long long)blockIdx.x * kEditWaves + wave;
  if (first >= slots) return;
  void *slot = scratch + (size_t)first * slot_bytes;
  int checked = -1;
  bool ok = true;
  for (long long w = first; w < work; w += slots) {
    const Pair p = pair_of(w, R, Q, false);
    const int b = __builtin_amdgcn_readfirstlane(p.b), i = __builtin_amdgcn_readfirstlane(p.i), j = __builtin_amdgcn_readfirstlane(p.j);
    if (b != checked) {
      ok = ops_item_ok(x_lens, b, R, L, y_lens, Q, Lq, lane);
      checked = b;
      if (!ok && status && lane == 0) status[b] = EDIT_BAD_ROW;
    }
    int32_t *xm = x_to_y + (size_t)w * L, *ym = y_to_x + (size_t)w * Lq;  // (w is the pair's row-major index)
    for (int q = lane; q < L; q += kEditLanes) xm[q] = -1;
    for (int q = lane; q < Lq; q += kEditLanes) ym[q] = -1;
    int32_t cnt[4] = {0, 0, 0, 0};
    if (ok) {
      const size_t xi = (size_t)b * R + i, yj = (size_t)b * Q + j;
      const int lx = __builtin_amdgcn_readfirstlane(x_lens[xi]), ly = __builtin_amdgcn_readfirstlane(y_lens[yj]);
      int key = key_trivial(lx, ly);
      if (lx != 0 && ly != 0) {
        const int32_t *xr = x + xi * (size_t)L, *yr = y + yj * (size_t)Lq;
        const bool x_strip = lx <= ly;
        const int32_t *strip = x_strip ? xr : yr, *stream = x_strip ? yr : xr;
        const int n = x_strip ? lx : ly, m = x_strip ? ly : lx;  // m <= max(L, Lq) rows of 64 words of the class: inside slot_bytes
        switch (strip_class(n)) {
          case 1: key = align_class<1>(strip, n, stream, m, lane, x_strip, slot, xm, ym); break;
          case 2: key = align_class<2>(strip, n, stream, m, lane, x_strip, slot, xm, ym); break;
          case 4: key = align_class<4>(strip, n, stream, m, lane, x_strip, slot, xm, ym); break;
          case 8: key = align_class<8>(strip, n, stream, m, lane, x_strip, slot, xm, ym); break;
          case 16: key = align_class<16>(strip, n, stream, m, lane, x_strip, slot, xm, ym); break;
          default: key = align_class<32>(strip, n, stream, m, lane, x_strip, slot, xm, ym);
        }
      }
      counts_of(key, lx, ly, cnt);
    }
    if (counts && lane == 0) {
      int32_t *o = counts + (size_t)w * 4;
      o[0] = cnt[0], o[1] = cnt[1], o[2] = cnt[2], o[3] = cnt[3];
    }
  }
}

// the checks both entry points share with ctcd_edit_distance, and the limit of the packed key.  -> CTCD_OK, or the code to return
static int ops_check(const std::string &f, int B, int R, int L, int Q, int Lq) {
  if ((L < Lq ? L : Lq) > kEditMaxStrip)
    return edit_fail(CTCD_EUNSUPPORTED, (f + "min(L, Lq) > 2048: the shorter row of a pair lives in one wave's registers, 32 columns per lane").c_str());
  if ((L < Lq ? Lq : L) > kOpsMaxDim)
    return edit_fail(CTCD_EUNSUPPORTED, (f + "max(L, Lq) > 262144: the packed key (distance * 4096 + substitutions) would leave int32").c_str());
  if ((long long)B * R > 0x7fffffffLL || (long long)B * Q > 0x7fffffffLL) return edit_fail(CTCD_EUNSUPPORTED, (f + "too many rows for one launch").c_str());
  return CTCD_OK;
}
// ctcd_edit_distance's grid: ctcd_set_edit_grid's cap (at most 2^20 workgroups), or two workgroups per compute unit
static long long ops_grid(const EditDecoderInfo &inf, long long work) {
  const long long cap = inf.cap > 0 ? (inf.cap < (1ll << 20) ? inf.cap : (1ll << 20)) : (long long)(inf.cus > 0 ? inf.cus : 1) * (kEditWavesPerCu / kEditWaves);
  const long long grid = (work + kEditWaves - 1) / kEditWaves;
  return grid < 1 ? 1 : (grid > cap ? cap : grid);
}

}  // namespace ctcedit

using namespace ctcedit;

extern "C" {

int ctcd_edit_counts(ctcd_decoder *d, const int32_t *x, const int32_t *x_lens, int B, int R, int L, const int32_t *y, const int32_t *y_lens, int Q, int Lq,
                     int32_t *out, int32_t *status, void *stream) {
  const std::string f = "ctcd_edit_counts: ";
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
  if (const int rc = ops_check(f, B, R, L, Q, Lq)) return rc;
  const long long work = pairs_per_item(R, Q, pairwise) * B;
  ctcdev::DeviceGuard guard;
  if (guard.enter(inf.device) != hipSuccess) return edit_fail(CTCD_EHIP, (std::string("hipSetDevice: ") + hipGetErrorString(guard.err)).c_str());
  const long long grid = ops_grid(inf, work);  // (a pairwise call of one-row items has no pair and a diagonal to write)
  hipLaunchKernelGGL(edit_counts_kernel, dim3((unsigned)grid), dim3(kEditThreads), 0, (hipStream_t)stream, x, x_lens, B, R, L, y, y_lens, Q, Lq, work, out, status);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return edit_fail(CTCD_EHIP, (std::string("edit counts: ") + hipGetErrorString(e)).c_str());
  edit_note_pairs(d, work, grid);
  return CTCD_OK;
}

int ctcd_edit_align(ctcd_decoder *d, const int32_t *x, const int32_t *x_lens, int B, int R, int L, const int32_t *y, const int32_t *y_lens, int Q, int Lq,
                    int32_t *x_to_y, int32_t *y_to_x, int32_t *counts, int32_t *status, void *stream) {
  const std::string f = "ctcd_edit_align: ";
  if (!d) return edit_fail(CTCD_EINVAL, "decoder == NULL");
  if (!y) return edit_fail(CTCD_EINVAL, (f + "y == NULL: alignments are not provided in pairwise mode").c_str());
  if (B < 0 || R < 0 || L < 0 || Q < 0 || Lq < 0) return edit_fail(CTCD_EINVAL, (f + "B, R, L, Q, Lq >= 0 required").c_str());
  EditDecoderInfo inf;
  if (const int rc = edit_decoder_info(d, &inf)) return rc;
  if (B == 0 || R == 0 || Q == 0) {
    edit_note_pairs(d, 0, 0);
    edit_note_slots(d, 0);
    return CTCD_OK;
  }
  if (!x_lens || !y_lens || (!x && L > 0) || (!x_to_y && L > 0) || (!y_to_x && Lq > 0)) return edit_fail(CTCD_EINVAL, (f + "null tensor").c_str());
  if (const int rc = ops_check(f, B, R, L, Q, Lq)) return rc;
  const long long work = pairs_per_item(R, Q, false) * B;
  // a slot per wave in flight: the usual grid's waves, or as many as the budget holds
  long long slots = ops_grid(inf, work) * kEditWaves;
  slots = slots < work ? slots : work;
  const size_t slot_bytes = ops_slot_bytes(L, Lq);
  if (slot_bytes) {
    const long long budget = edit_budget(d) > 0 ? edit_budget(d) : kOpsDefaultScratch, fit = budget / (long long)slot_bytes;
    if (fit < 1)
      return edit_fail(CTCD_EUNSUPPORTED, (f + "one back-pointer slot of " + std::to_string(slot_bytes) + " bytes (max(L, Lq) rows of 64 words) does not fit the scratch budget of " +
                                           std::to_string(budget) + " bytes (ctcd_set_edit_scratch)").c_str());
    slots = slots < fit ? slots : fit;
  }
  const long long grid = (slots + kEditWaves - 1) / kEditWaves;
  ctcdev::DeviceGuard guard;
  if (guard.enter(inf.device) != hipSuccess) return edit_fail(CTCD_EHIP, (std::string("hipSetDevice: ") + hipGetErrorString(guard.err)).c_str());
  void *scratch = nullptr;
  if (slot_bytes)
    if (const int rc = edit_scratch(d, (size_t)slots * slot_bytes, &scratch)) return rc;
  hipLaunchKernelGGL(edit_align_kernel, dim3((unsigned)grid), dim3(kEditThreads), 0, (hipStream_t)stream, x, x_lens, R, L, y, y_lens, Q, Lq, work, (char *)scratch,
                     slot_bytes, slots, x_to_y, y_to_x, counts, status);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return edit_fail(CTCD_EHIP, (std::string("edit align: ") + hipGetErrorString(e)).c_str());
  edit_note_pairs(d, work, grid);
  edit_note_slots(d, slots);
  return CTCD_OK;
}

}  // extern "C"
