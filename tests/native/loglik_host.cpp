// Host twin of the CTC log-likelihood (ctcdecode_amd/csrc/loglik.h): the routines the kernel of loglik.hip compiles -- lse3 over
// exact_math.h's expf / logf, the cell, the end rule, the grid arithmetic -- and align.h's row validation, run sequentially, one
// hypothesis after the other, behind a C ABI.  Test infrastructure only.
#define CTC_EXACT_MATH_HOST_TABLES
#include "../../ctcdecode_amd/csrc/loglik.h"

namespace {
template <int DT>
int loglik_all(const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank, int log_input, const int32_t *tokens, const int32_t *lens, int R,
               int L_stride, float *out, int32_t *status) {
  const uint64_t *tbl = ctcmath::host_tables().w;
  int bad = 0;
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < R; ++r) {
      const size_t h = (size_t)b * R + r;
      const int32_t *y = tokens + h * L_stride;
      const int rc = log_input == 0 ? ctcloglik::loglik_row_host<DT, true>(probs, seq_lens, b, T, V, blank, y, lens[h], L_stride, tbl, out + h)
                                    : ctcloglik::loglik_row_host<DT, false>(probs, seq_lens, b, T, V, blank, y, lens[h], L_stride, tbl, out + h);
      if (rc) {
        if (status) status[b] = rc;  // (raised only)
        ++bad;
      }
    }
  return bad;
}
}  // namespace

// probs [B, T, V] of dtype 0 / 1 / 2 (f32 / f16 / bf16); log_input 0 (probabilities) or 1 (log-probabilities; raw logits come as the
// log-softmax rows).  tokens [B, R, L_stride], lens [B, R]; out [B, R], status [B] (raised, never cleared) or NULL.  Returns the
// number of invalid rows, -1 for bad arguments.
extern "C" int ctcloglik_host_loglik(const void *probs, int dtype, const int32_t *seq_lens, int B, int T, int V, int blank, int log_input, const int32_t *tokens,
                                     const int32_t *lens, int R, int L_stride, float *out, int32_t *status) {
  if (B < 0 || T < 0 || V < 1 || R < 0 || L_stride < 0 || blank < 0 || blank >= V || log_input < 0 || log_input > 1 || dtype < 0 || dtype > 2) return -1;
  if ((long long)B * R == 0) return 0;
  if (!lens || !out || (L_stride > 0 && !tokens) || (T > 0 && !probs)) return -1;
  if (dtype == ctcskip::kSkipF16) return loglik_all<ctcskip::kSkipF16>(probs, seq_lens, B, T, V, blank, log_input, tokens, lens, R, L_stride, out, status);
  if (dtype == ctcskip::kSkipBF16) return loglik_all<ctcskip::kSkipBF16>(probs, seq_lens, B, T, V, blank, log_input, tokens, lens, R, L_stride, out, status);
  return loglik_all<ctcskip::kSkipF32>(probs, seq_lens, B, T, V, blank, log_input, tokens, lens, R, L_stride, out, status);
}

extern "C" float ctcloglik_host_lse3(float v0, float v1, float v2) { return ctcloglik::lse3(v0, v1, v2, ctcmath::host_tables().w); }
extern "C" long long ctcloglik_host_units(long long rows, int cls) { return ctcloglik::loglik_units(rows, cls); }
extern "C" int ctcloglik_host_occupancy(int cls) { return ctcloglik::loglik_occupancy(cls); }
extern "C" long long ctcloglik_host_grid(long long units, long long cap, int cus, int cls) { return ctcloglik::loglik_grid(units, cap, cus, cls); }
