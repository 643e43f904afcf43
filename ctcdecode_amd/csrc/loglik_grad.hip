// loglik_grad.hip -- the gradient of the CTC log-likelihood of loglik_grad.h on the device, and its C ABI (include/ctcdecode_amd.h
// "Log-likelihood gradient").  A translation unit of its own, like posterior.hip, whose two walks and scratch slots it shares.
//   ctc_loglik_grad_kernel<DT, PROB, CLS>  one launch per row index r and class: launch r covers row r of every item, so no two
//                                          workgroups of a launch touch the same item's [T][V] slab, plain load-add-store is enough,
//                                          and an item's rows accumulate in launch order.  The walk over the rows, their classes (CLS)
//                                          and the walk over a row's frames are lattice_device.h's.  Pass 1 is posterior.hip's: every
//                                          frame's a goes to the slot, the walk ends with ll.  Before pass 2 the unit sorts the row's
//                                          (label, position) pairs once in LDS: every distinct label gets one owner thread and the chain
//                                          of its positions in ascending order.  Pass 2 walks b; behind each frame every lane forms
//                                          w * g of ALL its states, puts the labels' into a double-buffered LDS row of L floats and
//                                          folds its blank states into the blank's tree (lane, wave butterfly, waves).  One barrier
//                                          later -- the walk's own, so a frame's sums run behind the next frame's cells -- the
//                                          owners sum their chains and add the totals to grad.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "lattice_device.h"
#include "loglik_grad.h"

namespace ctcgrad {

using namespace ctcalign;
using ctcpost::g_step;
using ctcpost::mirrored_state;

// exact_math.h's tables, staged into LDS by every workgroup (as posterior.hip does)
static __device__ const uint64_t kExpTab[32] = CTC_EXP2F_TAB;
static __device__ const double kLogInvc[16] = CTC_LOGF_INVC;
static __device__ const double kLogLogc[16] = CTC_LOGF_LOGC;

constexpr unsigned kPosBits = 12, kPosMask = (1u << kPosBits) - 1u;  // a position (< 2047) and, above it, its chain's length

// the labels a unit of class CLS holds at most (S <= 64: 31; S <= 256 CLS: 128 CLS - 1), as the stride of its LDS rows
constexpr int lds_labels(int cls) { return cls == 0 ? 32 : 128 * cls; }

// what stands between a unit's LDS writes and their readers: the workgroup's barrier, or -- one wave -- program order
template <int WAVES> __device__ __forceinline__ void unit_sync() {
  if (WAVES > 1) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// floats [0, count) at p <- +0.0 by the unit's threads, 16-byte stores between the boundaries (zero_words with a 64-bit count)
__device__ __forceinline__ void zero_span(float *p, size_t count, int utid, int nt) {
  size_t head = (size_t)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
  if (head > count) head = count;
  const size_t body = (count - head) >> 2, tail0 = head + body * 4;
  if ((size_t)utid < head) p[utid] = 0.0f;
  const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 *q = reinterpret_cast<float4 *>(p + head);
  for (size_t i = (size_t)utid; i < body; i += (size_t)nt) q[i] = z;
  if ((size_t)utid < count - tail0) p[tail0 + (size_t)utid] = 0.0f;
}

// The unit's LDS for the reduction by label.
struct LabelRows {
  int32_t *rev;   // the reversed labels (pass 2 walks them)
  unsigned *ord;  // sorted by (label, position): the position, and in a chain's first entry its length << kPosBits
  int32_t *lab;   // the label of each sorted entry
  float *gb;      // two rows of `stride` floats: a frame's w * g by position, frame t in row t & 1
  float *bl;      // two rows of WAVES floats: the waves' blank totals of a frame
  int stride;
};

// Pass 1 (walk_row with FIRST): posterior.hip's -- a frame's a of the lane's states goes to the frame's row of S floats at al + t * S.
template <int NPL> struct ForwardRow {
  const uint64_t *tbl;
  float *al;
  int S;
  float ll;
  float v[NPL];

  __device__ __forceinline__ void first(int k, float, float a) { v[k] = a; }
  __device__ __forceinline__ float cell(int k, float lp, float stay, float p1, float p2, bool has2) {
    return v[k] = ctcloglik::cell_update(lp, stay, p1, has2 ? p2 : neg_inf(), tbl);
  }
  __device__ __forceinline__ void frame(int t, int s0, int) {
    float *row = al + (size_t)t * S + s0;
#pragma unroll
    for (int k = 0; k < NPL; ++k)
      if (s0 + k < S) row[k] = v[k];
  }
  // (the rows are read back by pass 2, by other lanes of the unit; the first launch's zeroes of grad lie before pass 2's sums)
  __device__ __forceinline__ void frames_done() { __threadfence(); }
  __device__ __forceinline__ void finish(float a_last, float a_before, int L, int) { ll = ctcloglik::end_value(L, a_last, a_before, tbl); }
};

// The row's (label, position) pairs in ascending order, by rank: entry i's rank is the number of pairs below it.  L^2 / threads
// broadcast reads of LDS, once per row, where the walks cost 2 n frames of a barrier each.  Then every chain's first entry counts it.
template <int WAVES> __device__ __forceinline__ void sort_labels(const LabelRows &m, int L, int utid) {
  constexpr int NT = 64 * WAVES;
  for (int i = utid; i < L; i += NT) {
    const int yi = m.rev[L - 1 - i];
    int rank = 0;
    for (int j = 0; j < L; ++j) {
      const int yj = m.rev[L - 1 - j];
      rank += (yj < yi || (yj == yi && j < i)) ? 1 : 0;
    }
    m.ord[rank] = (unsigned)i;
    m.lab[rank] = yi;
  }
  unit_sync<WAVES>();
  for (int j = utid; j < L; j += NT) {
    const int y = m.lab[j];
    if (j == 0 || m.lab[j - 1] != y) {
      int cnt = 1;
      while (j + cnt < L && m.lab[j + cnt] == y) ++cnt;
      m.ord[j] |= (unsigned)cnt << kPosBits;  // (no other thread looks at ord before the barrier)
    }
  }
  unit_sync<WAVES>();
}

// Pass 2 (walk_row with REV and FIRST, on the reversed labels): posterior.hip's cell, which is b; lane state s' is the row's state
// S - 1 - s'.  Every state forms w * g; behind a frame the lanes hand the values over and sum those of the frame before.
template <int WAVES, int NPL> struct BackwardGrad {
  const uint64_t *tbl;
  const float *al;
  int S, L, n, V, blank;
  float ll, w;
  float *slab;  // the item's [T][V] floats of grad
  bool first_launch;
  LabelRows m;
  int t;          // the frame the next cells belong to
  float an[NPL];  // its a of the lane's states (-inf: no such state)
  float gv[NPL];  // w * g of the frame just computed

  // frame tt's a of the lane's states: device-scope loads, behind pass 1's fence and the unit's barrier
  __device__ __forceinline__ void load(int tt, int s0) {
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int s = s0 + k;
      an[k] = neg_inf();
      if (s < S) an[k] = __hip_atomic_load(al + (size_t)tt * S + mirrored_state(S, s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __device__ __forceinline__ void note(int k, float lp, float b) { gv[k] = weighted(w, g_step(an[k], b, lp, ll, tbl)); }
  __device__ __forceinline__ void first(int k, float lp, float b) { note(k, lp, b); }
  __device__ __forceinline__ float cell(int k, float lp, float stay, float p1, float p2, bool has2) {
    const float b = ctcloglik::cell_update(lp, stay, p1, has2 ? p2 : neg_inf(), tbl);
    note(k, lp, b);
    return b;
  }
  // grad[tt][v] += x (the first launch found the slab zeroed by its own unit and stores); the only writer of the element in this launch
  __device__ __forceinline__ void emit(int tt, int v, float x) {
    float *q = slab + (size_t)tt * V + v;
    *q = first_launch ? x : *q + x;
  }
  // frame tt's totals from row p: every chain by its owner, the blank's by the unit's first thread
  __device__ __forceinline__ void reduce(int tt, int p, float blank_total, int utid) {
    const float *x = m.gb + p * m.stride;
    for (int j = utid; j < L; j += 64 * WAVES) {
      const unsigned e = m.ord[j];
      const int cnt = (int)(e >> kPosBits);
      if (cnt) {
        float s = x[e & kPosMask];
        for (int i = 1; i < cnt; ++i) s = s + x[m.ord[j + i] & kPosMask];
        emit(tt, m.lab[j], s);
      }
    }
    if (utid == 0) {
      if (WAVES > 1) {
        const float *wv = m.bl + p * WAVES;
        blank_total = (wv[0] + wv[1]) + (wv[WAVES > 1 ? 2 : 0] + wv[WAVES > 1 ? 3 : 0]);
      }
      emit(tt, blank, blank_total);
    }
  }
  __device__ __forceinline__ void frame(int tt, int s0, int lane) {
    const int p = tt & 1, utid = s0 / NPL;
    float *x = m.gb + p * m.stride;
#pragma unroll
    for (int k = 0; k < NPL; ++k) {
      const int s = s0 + k;
      if ((s & 1) && s < S) x[mirrored_state(S, s) >> 1] = gv[k];
    }
    // the blank's tree: the lane's states (beyond S they are +0.0), the wave's lanes, and -- in reduce() -- the waves
    float bt = lane_blank_tree<NPL>(gv, (s0 & 1) == 0);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) bt = bt + __shfl_xor(bt, d, 64);
    if (WAVES > 1 && lane == 0) m.bl[p * WAVES + (utid >> 6)] = bt;
    t = tt - 1;
    if (t >= 0) load(t, s0);
    if (WAVES == 1) {
      unit_sync<1>();
      reduce(tt, p, bt, utid);
    } else if (tt + 1 < n) {
      reduce(tt + 1, p ^ 1, 0.0f, utid);  // (behind the barrier that followed frame tt + 1; frame tt - 1 writes the row a barrier later)
    }
  }
  __device__ __forceinline__ void frames_done() {}
  __device__ __forceinline__ void finish(float, float, int, int utid) {
    if (WAVES > 1) reduce(0, 0, 0.0f, utid);  // (walk_row's barrier behind the last frame stands before this)
  }
};

// The rows of a launch (lattice_device.h walk_groups, R = 1: row b of the launch is item b's).
template <int DT, bool PROB> struct GradRows {
  const uint64_t *tbl;
  const void *probs;
  int T, V, blank;
  const int32_t *tokens;
  const float *weights;
  int L_stride;
  float *slot;  // the workgroup's scratch slot
  LabelRows m;  // the workgroup's LDS rows (the waves of class 0: 32 labels each)
  float *grad, *out_ll;
  bool first_launch;

  template <int WAVES> __device__ __forceinline__ float *begin(long long row, int utid) {
    float *slab = grad + (size_t)row * (size_t)T * (size_t)V;
    if (first_launch) zero_span(slab, (size_t)T * (size_t)V, utid, 64 * WAVES);
    return slab;
  }
  template <int WAVES, int NPL> __device__ __forceinline__ void run(long long row, int n, int L, float *al, const LabelRows &lm, int utid) {
    float *slab = begin<WAVES>(row, utid);
    const int32_t *tok = tokens + (size_t)row * L_stride;
    const int S = n_states(L);
    ForwardRow<NPL> f{tbl, al, S, 0.0f, {}};
    ctclattice::walk_row<WAVES, NPL, DT, PROB, false, true>(f, probs, (size_t)row * T, n, V, blank, tok, L, utid);
    if (utid == 0) out_ll[row] = f.ll;
    const float w = weights[row];
    if (!(f.ll > neg_inf()) || w == 0.0f) return;  // (the same on every thread of the unit) no alignment, or a term of +0.0 everywhere
    for (int i = utid; i < L; i += 64 * WAVES) lm.rev[i] = tok[L - 1 - i];
    unit_sync<WAVES>();  // (rev; a was fenced by every thread before the barrier that ends pass 1)
    sort_labels<WAVES>(lm, L, utid);
    BackwardGrad<WAVES, NPL> r{tbl, al, S, L, n, V, blank, f.ll, w, slab, first_launch, lm, n - 1, {}, {}};
    r.load(n - 1, utid * NPL);
    ctclattice::walk_row<WAVES, NPL, DT, PROB, true, true>(r, probs, (size_t)row * T, n, V, blank, lm.rev, L, utid);
  }
  __device__ __forceinline__ void short_row(long long row, int, int n, int L, int lane, int wave) {
    const LabelRows lm{m.rev + wave * 32, m.ord + wave * 32, m.lab + wave * 32, m.gb + wave * 64, m.bl, 32};
    run<1, 1>(row, n, L, slot + (size_t)wave * ctcpost::post_wave_floats(T), lm, lane);
  }
  template <int NPL> __device__ __forceinline__ void long_row(long long row, int, int n, int L, int tid) { run<kAlignWaves, NPL>(row, n, L, slot, m, tid); }
  // a row that runs no recurrence adds nothing; its log-likelihood is given
  template <int WAVES> __device__ __forceinline__ void no_row(long long row, float ll, int utid) {
    begin<WAVES>(row, utid);
    if (utid == 0) out_ll[row] = ll;
  }
};

template <int DT, bool PROB, int CLS>
__global__ void __launch_bounds__(kAlignThreads) ctc_loglik_grad_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens,
                                                                        const int32_t *lens, const float *weights, int L_stride, long long rows, char *scratch,
                                                                        size_t slot_bytes, float *grad, float *out_ll, int32_t *status, int first_launch) {
  constexpr int N = CLS == 0 ? kAlignWaves * lds_labels(0) : lds_labels(CLS);
  __shared__ uint64_t s_tbl[64];
  __shared__ int32_t s_rev[N], s_lab[N];
  __shared__ unsigned s_ord[N];
  __shared__ float s_gb[2 * N], s_bl[2 * kAlignWaves];
  const int tid = (int)threadIdx.x;
  if (tid < 32) s_tbl[tid] = kExpTab[tid];
  else if (tid < 48) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogInvc[tid - 32]);
  else if (tid < 64) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogLogc[tid - 48]);
  // (the first barrier of the walk stands between these stores and their readers)
  GradRows<DT, PROB> pol{s_tbl, probs, T, V, blank, tokens, weights, L_stride, reinterpret_cast<float *>(scratch + (size_t)blockIdx.x * slot_bytes),
                         LabelRows{s_rev, s_ord, s_lab, s_gb, s_bl, N}, grad, out_ll, first_launch != 0};
  ctclattice::walk_groups<CLS>(pol, seq_lens, T, V, blank, tokens, lens, 1, L_stride, rows, status);
}

}  // namespace ctcgrad

using namespace ctcgrad;

extern "C" {

int ctcd_ctc_loglik_grad(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *tokens,
                         const int32_t *lens, const float *weights, int R, int L_stride, float *out_grad, float *out_loglik, int32_t *status, void *stream) {
  ctcdev::DeviceGuard guard;
  AlignEntry en;
  const int rc = align_entry("ctcd_ctc_loglik_grad", d, probs, seq_lens, B, T, V, blank_id, log_input, tokens, lens, R, L_stride,
                             weights && out_loglik && (out_grad || T == 0), stream, &guard, &en);
  if (rc != CTCD_OK || en.rows == 0) return rc;
  // one launch per r covers row r of all B items: the slots, the grid and the groups are those of B rows
  const size_t slot = ctcpost::post_slot_bytes(T, L_stride);
  const long long grid = ctcpost::post_grid(B, ctcpost::post_budget(d), slot);
  void *scratch = nullptr;
  if (const int rc2 = ctcpost::post_scratch(d, (size_t)grid * slot, &scratch)) return rc2;
  ctcpost::post_note_grid(d, grid);
  const long long groups = align_groups(B);
  for (int r = 0; r < R; ++r) {
    const int32_t *tok = tokens ? tokens + (size_t)r * B * L_stride : nullptr;
    const hipError_t e = ctclattice::launch_classes(en.dtype, log_input == 0, T, L_stride, [&](auto dt, auto prob, auto cls) {
      constexpr int CLS = decltype(cls)::value;
      const long long g = CLS == 0 && grid > groups ? groups : grid;
      hipLaunchKernelGGL((ctc_loglik_grad_kernel<decltype(dt)::value, decltype(prob)::value, CLS>), dim3((unsigned)g), dim3(kAlignThreads), 0, (hipStream_t)stream,
                         en.probs, seq_lens, T, V, blank_id, tok, lens + (size_t)r * B, weights + (size_t)r * B, L_stride, (long long)B, (char *)scratch, slot, out_grad,
                         out_loglik + (size_t)r * B, status, r == 0 ? 1 : 0);
    });
    if (e != hipSuccess) return align_fail(CTCD_EHIP, (std::string("log-likelihood gradient: ") + hipGetErrorString(e)).c_str());
  }
  return CTCD_OK;
}

}  // extern "C"
