// posterior.hip -- the per-label CTC posteriors of posterior.h on the device, and their C ABI (include/ctcdecode_amd.h "Label
// posteriors").  A translation unit of its own, like align.hip and loglik.hip: it runs behind a decode on tensors that decode left in
// HBM, and no kernel of the other files sees it.
//   ctc_posterior_kernel<DT, PROB, CLS>  persistent workgroups of four waves, each with its own slot of the decoder's scratch.  The
//                                        walk over the rows, their classes (CLS) and the walk over a row's frames are
//                                        lattice_device.h's.  A row is walked twice.  Pass 1 is the log-likelihood's walk; it also
//                                        keeps every frame's a in the slot and ends with ll.  Pass 2 is the same walk on the reversed
//                                        labels (staged in LDS) over the frames in descending order, which is b: lane state s' is the
//                                        row's state S - 1 - s'.  Behind each frame it loads the next frame's a of its odd states,
//                                        and each odd cell forms g and updates its label's accumulators in registers; behind the
//                                        last frame the lanes write their labels' outputs and the unit zeroes the tails.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "lattice_device.h"
#include "posterior.h"

namespace ctcpost {

using namespace ctcalign;

// exact_math.h's tables, staged into LDS by every workgroup (Tables::w: [0, 32) exp2f, [32, 48) logf invc, [48, 64) logf logc)
static __device__ const uint64_t kExpTab[32] = CTC_EXP2F_TAB;
static __device__ const double kLogInvc[16] = CTC_LOGF_INVC;
static __device__ const double kLogLogc[16] = CTC_LOGF_LOGC;

// Pass 1 (walk_row with FIRST): loglik.hip's cell; a frame's values of the lane's states, NPL consecutive floats of the frame's row of
// S floats at al + t * S; behind the last frame the end rule.
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
  __device__ __forceinline__ void frames_done() { __threadfence(); }  // (the rows are read back by pass 2, by other lanes of the unit)
  __device__ __forceinline__ void finish(float a_last, float a_before, int L, int) { ll = ctcloglik::end_value(L, a_last, a_before, tbl); }
};

// Pass 2 (walk_row with REV and FIRST, on the reversed labels): the same cell, which is b.  Only the lane's odd states are labels'
// (S - 1 is even, so s' is odd where the row's state is): NL of them -- with one state per lane, the lane's state if it is odd.
template <int WAVES, int NPL> struct BackwardRow {
  static constexpr int NL = NPL == 1 ? 1 : NPL / 2;
  const uint64_t *tbl;
  const float *al;
  int S, L_stride;
  float ll;
  int32_t *peaks;
  float *occ, *conf;
  int t;          // the frame the next cells belong to
  float an[NL];   // its a of the lane's odd states (-inf: no such state)
  LabelAcc acc[NL];

  static __device__ __forceinline__ int odd_state(int s0, int j) { return NPL == 1 ? s0 : s0 + 2 * j + 1; }
  // frame tt's a of the lane's odd states: device-scope loads, behind pass 1's fence and the unit's barrier
  __device__ __forceinline__ void load(int tt, int s0) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int s = odd_state(s0, j);
      an[j] = neg_inf();
      if ((s & 1) && s < S) an[j] = __hip_atomic_load(al + (size_t)tt * S + mirrored_state(S, s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __device__ __forceinline__ void note(int k, float lp, float b) {
    if (NPL == 1 || (k & 1)) {
      const int j = NPL == 1 ? 0 : k >> 1;
      acc_update(acc[j], t, g_step(an[j], b, lp, ll, tbl), lp, tbl);
    }
  }
  __device__ __forceinline__ void first(int k, float lp, float b) { note(k, lp, b); }
  __device__ __forceinline__ float cell(int k, float lp, float stay, float p1, float p2, bool has2) {
    const float b = ctcloglik::cell_update(lp, stay, p1, has2 ? p2 : neg_inf(), tbl);
    note(k, lp, b);
    return b;
  }
  __device__ __forceinline__ void frame(int tt, int s0, int) {
    t = tt - 1;
    if (t >= 0) load(t, s0);
  }
  __device__ __forceinline__ void frames_done() {}
  __device__ __forceinline__ void finish(float, float, int L, int utid) {
    const int s0 = utid * NPL;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int s = odd_state(s0, j);
      if ((s & 1) && s < S) {
        const int i = mirrored_state(S, s) >> 1;
        peaks[i] = acc[j].peak;
        occ[i] = acc[j].occ;
        conf[i] = acc_confidence(acc[j]);
      }
    }
    zero_tails(peaks, occ, conf, L, L_stride, utid);
  }
  // positions [from, L_stride) of the three outputs <- 0
  static __device__ __forceinline__ void zero_tails(int32_t *peaks, float *occ, float *conf, int from, int L_stride, int utid) {
    ctclattice::zero_words(peaks + from, L_stride - from, utid, 64 * WAVES);
    ctclattice::zero_words(reinterpret_cast<int32_t *>(occ) + from, L_stride - from, utid, 64 * WAVES);
    ctclattice::zero_words(reinterpret_cast<int32_t *>(conf) + from, L_stride - from, utid, 64 * WAVES);
  }
};

// The rows of a launch (lattice_device.h walk_groups): where a row's labels, scratch and outputs lie.
template <int DT, bool PROB> struct PosteriorRows {
  const uint64_t *tbl;
  const void *probs;
  int T, V, blank;
  const int32_t *tokens;
  int L_stride;
  float *slot;     // the workgroup's scratch slot
  int32_t *rev;    // LDS: the reversed labels of the rows in flight
  int32_t *out_pk;
  float *out_occ, *out_conf, *out_ll;

  template <int WAVES, int NPL> __device__ __forceinline__ void run(long long row, int b, int n, int L, float *al, int32_t *rv, int utid) {
    const int32_t *tok = tokens + (size_t)row * L_stride;
    const size_t o = (size_t)row * L_stride;
    const int S = n_states(L);
    ForwardRow<NPL> f{tbl, al, S, 0.0f, {}};
    ctclattice::walk_row<WAVES, NPL, DT, PROB, false, true>(f, probs, (size_t)b * T, n, V, blank, tok, L, utid);
    if (utid == 0) out_ll[row] = f.ll;
    if (L == 0 || !(f.ll > neg_inf())) {  // (the same on every thread of the unit) no labels, or no alignment: the outputs are 0
      BackwardRow<WAVES, NPL>::zero_tails(out_pk + o, out_occ + o, out_conf + o, 0, L_stride, utid);
      return;
    }
    for (int i = utid; i < L; i += 64 * WAVES) rv[i] = tok[L - 1 - i];
    if (WAVES > 1) __syncthreads();  // (rv; a was fenced by every thread before the barrier that ends pass 1)
    BackwardRow<WAVES, NPL> r{tbl, al, S, L_stride, f.ll, out_pk + o, out_occ + o, out_conf + o, n - 1, {}, {}};
#pragma unroll
    for (int j = 0; j < BackwardRow<WAVES, NPL>::NL; ++j) acc_init(r.acc[j]);
    r.load(n - 1, utid * NPL);
    ctclattice::walk_row<WAVES, NPL, DT, PROB, true, true>(r, probs, (size_t)b * T, n, V, blank, rv, L, utid);
  }
  __device__ __forceinline__ void short_row(long long row, int b, int n, int L, int lane, int wave) {
    run<1, 1>(row, b, n, L, slot + (size_t)wave * post_wave_floats(T), rev + wave * 32, lane);
  }
  template <int NPL> __device__ __forceinline__ void long_row(long long row, int b, int n, int L, int tid) { run<kAlignWaves, NPL>(row, b, n, L, slot, rev, tid); }
  // the outputs zero, the log-likelihood given
  template <int WAVES> __device__ __forceinline__ void no_row(long long row, float ll, int utid) {
    const size_t o = (size_t)row * L_stride;
    BackwardRow<WAVES, 1>::zero_tails(out_pk + o, out_occ + o, out_conf + o, 0, L_stride, utid);
    if (utid == 0) out_ll[row] = ll;
  }
};

template <int DT, bool PROB, int CLS>
__global__ void __launch_bounds__(kAlignThreads) ctc_posterior_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens,
                                                                      const int32_t *lens, int R, int L_stride, long long rows, char *scratch, size_t slot_bytes,
                                                                      int32_t *out_pk, float *out_occ, float *out_conf, float *out_ll, int32_t *status) {
  __shared__ uint64_t s_tbl[64];
  // the reversed labels: 32 words for each of four one-wave rows (L <= 31), or the (L <= 128 * CLS - 1) labels of the workgroup's row
  __shared__ int32_t s_rev[CLS == 0 ? 128 : 128 * CLS];
  const int tid = (int)threadIdx.x;
  if (tid < 32) s_tbl[tid] = kExpTab[tid];
  else if (tid < 48) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogInvc[tid - 32]);
  else if (tid < 64) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogLogc[tid - 48]);
  // (the first barrier of the walk stands between these stores and their readers)
  PosteriorRows<DT, PROB> pol{s_tbl, probs, T, V, blank, tokens, L_stride, reinterpret_cast<float *>(scratch + (size_t)blockIdx.x * slot_bytes), s_rev,
                              out_pk, out_occ, out_conf, out_ll};
  ctclattice::walk_groups<CLS>(pol, seq_lens, T, V, blank, tokens, lens, R, L_stride, rows, status);
}

}  // namespace ctcpost

using namespace ctcpost;

extern "C" {

int ctcd_ctc_posteriors(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *tokens,
                        const int32_t *lens, int R, int L_stride, int32_t *out_peaks, float *out_occupancy, float *out_confidence, float *out_loglik,
                        int32_t *status, void *stream) {
  ctcdev::DeviceGuard guard;
  AlignEntry en;
  const int rc = align_entry("ctcd_ctc_posteriors", d, probs, seq_lens, B, T, V, blank_id, log_input, tokens, lens, R, L_stride,
                             out_loglik && (L_stride == 0 || (out_peaks && out_occupancy && out_confidence)), stream, &guard, &en);
  if (rc != CTCD_OK || en.rows == 0) return rc;
  const size_t slot = post_slot_bytes(T, L_stride);
  const long long grid = post_grid(en.rows, post_budget(d), slot);
  void *scratch = nullptr;
  if (const int rc2 = post_scratch(d, (size_t)grid * slot, &scratch)) return rc2;
  post_note_grid(d, grid);
  // class 0 takes a group of four rows per workgroup at a time (at most the groups), the other classes one row
  const long long groups = align_groups(en.rows);
  const hipError_t e = ctclattice::launch_classes(en.dtype, log_input == 0, T, L_stride, [&](auto dt, auto prob, auto cls) {
    const long long g = decltype(cls)::value == 0 && grid > groups ? groups : grid;
    hipLaunchKernelGGL((ctc_posterior_kernel<decltype(dt)::value, decltype(prob)::value, decltype(cls)::value>), dim3((unsigned)g), dim3(kAlignThreads), 0,
                       (hipStream_t)stream, en.probs, seq_lens, T, V, blank_id, tokens, lens, R, L_stride, en.rows, (char *)scratch, slot, out_peaks, out_occupancy,
                       out_confidence, out_loglik, status);
  });
  return e == hipSuccess ? CTCD_OK : align_fail(CTCD_EHIP, (std::string("label posteriors: ") + hipGetErrorString(e)).c_str());
}

}  // extern "C"
