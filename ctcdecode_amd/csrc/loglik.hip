// loglik.hip -- the CTC log-likelihood of loglik.h on the device, and its C ABI (include/ctcdecode_amd.h "CTC log-likelihood").  A
// translation unit of its own, like align.hip: it runs behind a decode on tensors that decode left in HBM, and no kernel of
// ctcdecode_amd.hip, decode_kernels.hip or align.hip sees it.
//   ctc_loglik_kernel<DT, PROB, CLS>  persistent workgroups of four waves.  The walk over the rows, their classes (CLS) and the walk
//                                     over a row's frames are lattice_device.h's, shared with align.hip; here are the cell (lse3 on
//                                     exact_math.h's tables, staged into LDS) and the end rule.  No back-pointers and no scratch: the
//                                     only memory a row writes is its float.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "lattice_device.h"
#include "loglik.h"

namespace ctcloglik {

using namespace ctcalign;

// exact_math.h's tables, staged into LDS by every workgroup (Tables::w: [0, 32) exp2f, [32, 48) logf invc, [48, 64) logf logc)
static __device__ const uint64_t kExpTab[32] = CTC_EXP2F_TAB;
static __device__ const double kLogInvc[16] = CTC_LOGF_INVC;
static __device__ const double kLogLogc[16] = CTC_LOGF_LOGC;

// One row's walk (lattice_device.h walk_row): a frame's NPL cells of a lane are independent chains of max3, two expf, one logf and
// two additions, and the compiler interleaves them; nothing is kept of a frame; behind the last one the end rule, on every thread.
struct LoglikRow {
  const uint64_t *tbl;
  float ll;

  __device__ __forceinline__ float cell(int, float lp, float stay, float p1, float p2, bool has2) { return cell_update(lp, stay, p1, has2 ? p2 : neg_inf(), tbl); }
  __device__ __forceinline__ void frame(int, int, int) {}
  __device__ __forceinline__ void frames_done() {}
  __device__ __forceinline__ void finish(float a_last, float a_before, int L, int) { ll = end_value(L, a_last, a_before, tbl); }
};

// The rows of a launch (lattice_device.h walk_groups): a row's float, written by the first thread of the unit that ran it.
template <int DT, bool PROB> struct LoglikRows {
  const uint64_t *tbl;
  const void *probs;
  int T, V, blank;
  const int32_t *tokens;
  int L_stride;
  float *out;

  template <int WAVES, int NPL> __device__ __forceinline__ void run(long long row, int b, int n, int L, int utid) {
    LoglikRow r{tbl, 0.0f};
    ctclattice::walk_row<WAVES, NPL, DT, PROB>(r, probs, (size_t)b * T, n, V, blank, tokens + (size_t)row * L_stride, L, utid);
    if (utid == 0) out[row] = r.ll;
  }
  __device__ __forceinline__ void short_row(long long row, int b, int n, int L, int lane, int) { run<1, 1>(row, b, n, L, lane); }
  template <int NPL> __device__ __forceinline__ void long_row(long long row, int b, int n, int L, int tid) { run<kAlignWaves, NPL>(row, b, n, L, tid); }
  template <int WAVES> __device__ __forceinline__ void no_row(long long row, float ll, int utid) {
    if (utid == 0) out[row] = ll;
  }
};

template <int DT, bool PROB, int CLS>
__global__ void __launch_bounds__(kAlignThreads) ctc_loglik_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens,
                                                                   const int32_t *lens, int R, int L_stride, long long rows, float *out, int32_t *status) {
  __shared__ uint64_t s_tbl[64];
  const int tid = (int)threadIdx.x;
  if (tid < 32) s_tbl[tid] = kExpTab[tid];
  else if (tid < 48) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogInvc[tid - 32]);
  else if (tid < 64) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogLogc[tid - 48]);
  // (the first barrier of the walk stands between these stores and their readers)
  LoglikRows<DT, PROB> pol{s_tbl, probs, T, V, blank, tokens, L_stride, out};
  ctclattice::walk_groups<CLS>(pol, seq_lens, T, V, blank, tokens, lens, R, L_stride, rows, status);
}

}  // namespace ctcloglik

using namespace ctcloglik;

extern "C" {

int ctcd_ctc_loglik(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *tokens,
                    const int32_t *lens, int R, int L_stride, float *out_loglik, int32_t *status, void *stream) {
  ctcdev::DeviceGuard guard;
  AlignEntry en;
  const int rc = align_entry("ctcd_ctc_loglik", d, probs, seq_lens, B, T, V, blank_id, log_input, tokens, lens, R, L_stride, out_loglik != nullptr, stream, &guard, &en);
  if (rc != CTCD_OK || en.rows == 0) return rc;
  LoglikDecoderInfo linf;
  if (const int rc2 = loglik_decoder_info(d, &linf)) return rc2;
  // no scratch binds the grids: each class's own (loglik.h loglik_grid); the largest of them is noted
  long long widest = 0;
  const hipError_t e = ctclattice::launch_classes(en.dtype, log_input == 0, T, L_stride, [&](auto dt, auto prob, auto cls) {
    constexpr int CLS = decltype(cls)::value;
    const long long grid = loglik_grid(loglik_units(en.rows, CLS), linf.cap, linf.cus, CLS);
    if (grid > widest) widest = grid;
    hipLaunchKernelGGL((ctc_loglik_kernel<decltype(dt)::value, decltype(prob)::value, CLS>), dim3((unsigned)grid), dim3(kAlignThreads), 0, (hipStream_t)stream,
                       en.probs, seq_lens, T, V, blank_id, tokens, lens, R, L_stride, en.rows, out_loglik, status);
  });
  loglik_note_grid(d, widest);
  return e == hipSuccess ? CTCD_OK : align_fail(CTCD_EHIP, (std::string("log-likelihood: ") + hipGetErrorString(e)).c_str());
}

}  // extern "C"
