// loglik.hip -- the CTC log-likelihood of loglik.h on the device, and its C ABI (include/ctcdecode_amd.h "CTC log-likelihood").  A
// translation unit of its own, like align.hip: it runs behind a decode on tensors that decode left in HBM, and no kernel of
// ctcdecode_amd.hip, decode_kernels.hip or align.hip sees it.
//   ctc_loglik_kernel<DT, PROB, CLS>  persistent workgroups of four waves; the register layout and the row classes are align.hip's
//                                     (DESIGN.md 2h): a group of four consecutive rows that all fit a wave (S <= 64) runs them side by
//                                     side, one per wave, without a barrier (CLS 0: workgroup g takes the groups g, g + grid, ...); the
//                                     rows of any other group run on a whole workgroup each, 1, 4 or 16 states per lane (CLS: workgroup g
//                                     takes the rows g, g + grid, ...), one barrier per frame.  No back-pointers and no scratch: the only
//                                     memory a row writes is its float.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "loglik.h"

namespace ctcloglik {

using namespace ctcalign;

// exact_math.h's tables, staged into LDS by every workgroup (Tables::w: [0, 32) exp2f, [32, 48) logf invc, [48, 64) logf logc)
static __device__ const uint64_t kExpTab[32] = CTC_EXP2F_TAB;
static __device__ const double kLogInvc[16] = CTC_LOGF_INVC;
static __device__ const double kLogLogc[16] = CTC_LOGF_LOGC;

// One hypothesis on one unit: WAVES = 1 (a wave, utid = its lane) or kAlignWaves (the workgroup, utid = the thread), NPL states per
// lane -- lane u holds states u * NPL .. u * NPL + NPL - 1 in registers, so that the neighbours s - 1 and s - 2 of all but a lane's
// first two states are its own.  The others come from the lane before it (__shfl_up) and, at a wave's first lane, from the wave before
// it through `xch` (two floats per wave and frame parity, written behind each frame, one barrier per frame).  A frame's NPL cells of a
// lane read only the frame before: they are independent chains of max3, two expf, one logf and two additions, and the compiler
// interleaves them.  The row was validated by the caller: 0 <= L <= n, n >= 1, S = 2L + 1 <= 64 * WAVES * NPL, every label in [0, V) and
// no blank.  Returns the row's log-likelihood in thread 0 of the unit.
template <int WAVES, int NPL, int DT, bool PROB>
__device__ __forceinline__ float loglik_row(const void *probs, size_t row0, int n, int V, int blank, const int32_t *tok, int L, float *xch, float *fin,
                                            const uint64_t *tbl, int utid) {
  constexpr int CH = NPL == 1 ? 8 : (NPL == 4 ? 4 : 2);  // frames whose log-probabilities are in flight while a chunk is computed
  const int lane = utid & 63, wave = utid >> 6;
  const int S = n_states(L), s0 = utid * NPL;
  // the lane's states: the column each gathers, and which of them have the third predecessor (frame-invariant).  States at or beyond
  // S gather the blank's column and compute on: no state below them ever reads them, and the end rule looks below them.
  constexpr unsigned kElem = DT == ctcskip::kSkipF32 ? 4u : 2u;
  unsigned zo[NPL];  // (byte offsets inside a frame's row, 32 bits: a frame's address is its uniform base plus these)
  unsigned has2 = 0u;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int s = s0 + k;
    zo[k] = (unsigned)blank * kElem;
    if (s < S) {
      if (s & 1) zo[k] = (unsigned)tok[s >> 1] * kElem;
      if (state_skips(tok, s)) has2 |= 1u << k;
    }
  }
  auto load = [&](float(&dst)[NPL], int t) {  // frame t's values as they lie in memory (a frame at or beyond n: frame n - 1's, unused)
    const char *fr = (const char *)probs + (row0 + (size_t)(t < n ? t : n - 1)) * (size_t)V * kElem;
#pragma unroll
    for (int k = 0; k < NPL; ++k) dst[k] = ctcskip::widen_at<DT>(fr + (size_t)zo[k], 0);
  };
  auto convert = [&](float(&v)[NPL]) {
    if (PROB) {
#pragma unroll
      for (int k = 0; k < NPL; ++k) v[k] = prob_to_lp(v[k]);
    }
  };
  // this frame's last two states of the wave, for the wave behind it
  float a[NPL];
  auto publish = [&](int par) {
    if (WAVES > 1) {
      const float before = NPL >= 2 ? a[NPL >= 2 ? NPL - 2 : 0] : __shfl_up(a[0], 1, 64);
      if (lane == 63) {
        xch[(par * WAVES + wave) * 2] = a[NPL - 1];
        xch[(par * WAVES + wave) * 2 + 1] = before;
      }
      __syncthreads();
    }
  };

  float cur[CH][NPL], nxt[CH][NPL];
  load(cur[0], 0);
  convert(cur[0]);
#pragma unroll
  for (int k = 0; k < NPL; ++k) a[k] = (s0 + k < 2 && s0 + k < S) ? cur[0][k] : neg_inf();
  publish(0);
#pragma unroll
  for (int c = 0; c < CH; ++c) load(cur[c], 1 + c);
#pragma unroll
  for (int c = 0; c < CH; ++c) convert(cur[c]);
  for (int t0 = 1; t0 < n; t0 += CH) {
#pragma unroll
    for (int c = 0; c < CH; ++c) load(nxt[c], t0 + CH + c);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int t = t0 + c;
      if (t < n) {  // (the same for every lane of the unit)
        // states s0 - 1 and s0 - 2 of frame t - 1
        float a_in, b_in;
        if (NPL == 1) {
          a_in = __shfl_up(a[0], 1, 64);
          b_in = __shfl_up(a[0], 2, 64);
        } else {
          a_in = __shfl_up(a[NPL - 1], 1, 64);
          b_in = __shfl_up(a[NPL >= 2 ? NPL - 2 : 0], 1, 64);
        }
        if (WAVES > 1 && wave > 0) {
          const int at = (((t - 1) & 1) * WAVES + wave - 1) * 2;
          if (lane == 0) {
            a_in = xch[at];
            b_in = xch[at + 1];
          }
          if (NPL == 1 && lane == 1) b_in = xch[at];
        }
        if (utid == 0) a_in = neg_inf();  // (state 0 has no predecessor but itself)
        float na[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
          const float p1 = k >= 1 ? a[k >= 1 ? k - 1 : 0] : a_in;
          const float p2 = k >= 2 ? a[k >= 2 ? k - 2 : 0] : (k == 1 ? a_in : b_in);
          na[k] = cell_update(cur[c][k], a[k], p1, ((has2 >> k) & 1u) ? p2 : neg_inf(), tbl);
        }
#pragma unroll
        for (int k = 0; k < NPL; ++k) a[k] = na[k];
        publish(t & 1);
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
      for (int k = 0; k < NPL; ++k) cur[c][k] = nxt[c][k];
      convert(cur[c]);
    }
  }
  // the end rule: a[n-1][S-1] and a[n-1][S-2], from the lanes that hold them
  float mine1 = 0.0f, mine2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    if (s0 + k == S - 1) mine1 = a[k];
    if (s0 + k == S - 2) mine2 = a[k];
  }
  float a_last, a_before = 0.0f;
  if (WAVES > 1) {
    if (s0 <= S - 1 && S - 1 < s0 + NPL) fin[0] = mine1;
    if (s0 <= S - 2 && S - 2 < s0 + NPL) fin[1] = mine2;
    __syncthreads();
    a_last = fin[0];
    if (L >= 1) a_before = fin[1];
  } else {
    a_last = __shfl(mine1, (S - 1) / NPL, 64);
    if (L >= 1) a_before = __shfl(mine2, (S - 2) / NPL, 64);
  }
  return end_value(L, a_last, a_before, tbl);
}

// what a wave found out about its row of the group
enum : int { kRowNone = -1, kRowInvalid = -2, kRowNoPath = -3 };  // else: L, a valid row that runs the recurrence (0 <= L <= n, n >= 1)

// The four classes of align.hip, each a kernel of its own (CLS), so that each gets the registers its class needs and no more: 0 = the
// rows of a group of four that all fit a wave (S <= 64, and the rows that run no recurrence), one per wave side by side; 1 / 4 / 16 =
// the rows of every other group, on the whole workgroup with that many states per lane (rows of such a group that run no recurrence:
// class 1).  Every kernel walks all rows and classes their groups alike; a row is written by exactly one of them.
template <int DT, bool PROB, int CLS>
__global__ void __launch_bounds__(kAlignThreads) ctc_loglik_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens,
                                                                   const int32_t *lens, int R, int L_stride, long long rows, float *out, int32_t *status) {
  __shared__ uint64_t s_tbl[64];
  __shared__ float s_xch[2 * kAlignWaves * 2];
  __shared__ float s_fin[2];
  __shared__ int s_row[kAlignWaves];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 32) s_tbl[tid] = kExpTab[tid];
  else if (tid < 48) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogInvc[tid - 32]);
  else if (tid < 64) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogLogc[tid - 48]);
  // (the first barrier of the loop below stands between these stores and their readers)
  const long long units = loglik_units(rows, CLS);
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const long long g = CLS == 0 ? u : u / kAlignWaves;
    // wave w looks at row 4g + w: its length against L_stride, then its labels against the vocabulary
    const long long h = g * kAlignWaves + wave;
    int what = kRowNone;
    if (h < rows) {
      const int b = (int)(h / R), len = lens[h];
      bool ok = len_ok(len, L_stride);
      if (ok) {
        const int32_t *y = tokens + (size_t)h * L_stride;
        bool bad = false;
        for (int i = lane; i < len; i += 64) bad |= !label_ok(y[i], V, blank);
        ok = __ballot(bad) == 0ull;
      }
      const int n = ctcskip::clamped_len(seq_lens, b, T);
      what = !ok ? kRowInvalid : ((n == 0 || len > n) ? kRowNoPath : len);
      if (!ok && status && lane == 0) status[b] = ALIGN_BAD_ROW;  // (raised only)
    }
    if (lane == 0) s_row[wave] = what;
    __syncthreads();
    bool all_short = true;
#pragma unroll
    for (int w = 0; w < kAlignWaves; ++w) all_short = all_short && n_states(s_row[w]) <= 64;  // (the negative codes count as short)
    if (CLS == 0) {
      if (all_short && h < rows) {
        const int b = (int)(h / R), n = ctcskip::clamped_len(seq_lens, b, T);
        float ll;
        if (what < 0)
          ll = what == kRowInvalid || (n == 0 && lens[h] == 0) ? 0.0f : neg_inf();
        else
          ll = loglik_row<1, 1, DT, PROB>(probs, (size_t)b * T, n, V, blank, tokens + (size_t)h * L_stride, what, s_xch, s_fin, s_tbl, lane);
        if (lane == 0) out[h] = ll;
      }
    } else if (!all_short) {
      const int code = s_row[(int)(u % kAlignWaves)];
      const int b = (int)(u / R), n = ctcskip::clamped_len(seq_lens, b, T);
      if (code < 0) {
        if (CLS == 1 && tid == 0) out[u] = code == kRowInvalid || (n == 0 && lens[u] == 0) ? 0.0f : neg_inf();
      } else if (align_npl(n_states(code)) == CLS) {  // (the launcher refuses shapes whose rows can exceed kAlignMaxStates)
        const float ll = loglik_row<kAlignWaves, CLS == 0 ? 1 : CLS, DT, PROB>(probs, (size_t)b * T, n, V, blank, tokens + (size_t)u * L_stride, code, s_xch, s_fin,
                                                                             s_tbl, tid);
        if (tid == 0) out[u] = ll;
      }
    }
    __syncthreads();  // (s_row, s_xch and s_fin belong to the next unit)
  }
}

namespace {
struct LoglikDeviceGuard {  // the caller's current device is put back on exit (as every entry point of ctcdecode_amd.hip does)
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit LoglikDeviceGuard(int dev) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != dev) prev = cur;
    if (cur != dev) err = hipSetDevice(dev);
  }
  ~LoglikDeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// the kernels of the classes the shape allows (S <= 2 * min(L_stride, T) + 1), one behind the other on the stream; *widest: the
// largest grid among them
template <int DT, bool PROB>
hipError_t launch(long long cap, int cus, hipStream_t s, const void *probs, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens, const int32_t *lens,
                  int R, int L_stride, long long rows, float *out, int32_t *status, long long *widest) {
  const int smax = n_states(align_lmax(T, L_stride));
  *widest = 0;
#define CTC_LOGLIK_CLASS(CLS)                                                                                                                              \
  do {                                                                                                                                                     \
    const long long grid = loglik_grid(loglik_units(rows, CLS), cap, cus, CLS);                                                                            \
    if (grid > *widest) *widest = grid;                                                                                                                    \
    hipLaunchKernelGGL((ctc_loglik_kernel<DT, PROB, CLS>), dim3((unsigned)grid), dim3(kAlignThreads), 0, s, probs, seq_lens, T, V, blank, tokens, lens, R, \
                       L_stride, rows, out, status);                                                                                                       \
  } while (0)
  CTC_LOGLIK_CLASS(0);
  if (smax > 64) CTC_LOGLIK_CLASS(1);
  if (smax > kAlignThreads) CTC_LOGLIK_CLASS(4);
  if (smax > kAlignThreads * 4) CTC_LOGLIK_CLASS(16);
#undef CTC_LOGLIK_CLASS
  return hipGetLastError();
}
}  // namespace
}  // namespace ctcloglik

using namespace ctcloglik;

extern "C" {

int ctcd_ctc_loglik(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *tokens,
                    const int32_t *lens, int R, int L_stride, float *out_loglik, int32_t *status, void *stream) {
  if (!d) return align_fail(CTCD_EINVAL, "decoder == NULL");
  if (B < 0 || T < 0 || V < 1 || R < 0 || L_stride < 0) return align_fail(CTCD_EINVAL, "ctcd_ctc_loglik: B, T, R, L_stride >= 0 and V >= 1 required");
  if (blank_id < 0 || blank_id >= V) return align_fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (log_input < 0 || log_input > 2) return align_fail(CTCD_EINVAL, "ctcd_ctc_loglik: log_input must be 0, 1 or 2");
  const long long rows = (long long)B * R;
  if (rows == 0) return CTCD_OK;
  if (!tokens && L_stride > 0) return align_fail(CTCD_EINVAL, "ctcd_ctc_loglik: null tensor");
  if (!lens || !out_loglik || (T > 0 && !probs)) return align_fail(CTCD_EINVAL, "ctcd_ctc_loglik: null tensor");
  if (align_lmax(T, L_stride) > kAlignMaxLabels)
    return align_fail(CTCD_EUNSUPPORTED, "ctcd_ctc_loglik: rows of more than 2047 labels (min(L_stride, T) > 2047) are not built");
  if (V > (1 << 28)) return align_fail(CTCD_EUNSUPPORTED, "ctcd_ctc_loglik: V > 2^28");  // (a row's byte offsets are 32 bits)
  if (rows > 0x7fffffffLL) return align_fail(CTCD_EUNSUPPORTED, "ctcd_ctc_loglik: too many rows for one launch");
  AlignDecoderInfo inf;
  if (const int rc = align_decoder_info(d, &inf)) return rc;
  LoglikDecoderInfo linf;
  if (const int rc = loglik_decoder_info(d, &linf)) return rc;
  LoglikDeviceGuard guard(inf.device);
  if (guard.err != hipSuccess) return align_fail(CTCD_EHIP, (std::string("hipSetDevice: ") + hipGetErrorString(guard.err)).c_str());
  int dt = inf.in_dtype;
  if (log_input == 2 && T > 0) {  // raw logits: the log-softmax pass into the decoder's float32 rows, then log-probabilities
    const float *rows32 = nullptr;
    if (const int rc = align_lsm_rows(d, probs, seq_lens, B, T, V, stream, &rows32)) return rc;
    probs = rows32;
    dt = CTCD_DTYPE_F32;
  }
  hipStream_t s = (hipStream_t)stream;
  const bool prob = log_input == 0;
  long long widest = 0;
  hipError_t e;
#define CTC_LOGLIK_LAUNCH(DT, PROB) \
  launch<DT, PROB>(linf.cap, linf.cus, s, probs, seq_lens, T, V, blank_id, tokens, lens, R, L_stride, rows, out_loglik, status, &widest)
  if (dt == CTCD_DTYPE_F16) e = prob ? CTC_LOGLIK_LAUNCH(ctcskip::kSkipF16, true) : CTC_LOGLIK_LAUNCH(ctcskip::kSkipF16, false);
  else if (dt == CTCD_DTYPE_BF16) e = prob ? CTC_LOGLIK_LAUNCH(ctcskip::kSkipBF16, true) : CTC_LOGLIK_LAUNCH(ctcskip::kSkipBF16, false);
  else e = prob ? CTC_LOGLIK_LAUNCH(ctcskip::kSkipF32, true) : CTC_LOGLIK_LAUNCH(ctcskip::kSkipF32, false);
#undef CTC_LOGLIK_LAUNCH
  loglik_note_grid(d, widest);
  return e == hipSuccess ? CTCD_OK : align_fail(CTCD_EHIP, (std::string("log-likelihood: ") + hipGetErrorString(e)).c_str());
}

}  // extern "C"
