// Host twin of the label posteriors (ctcdecode_amd/csrc/posterior.h): the routines the kernel of posterior.hip compiles -- e80, the g
// step, the accumulator update, the slot and grid arithmetic, over loglik.h's lse3 and cell -- and align.h's row validation, run
// sequentially, one hypothesis after the other, behind a C ABI.  Test infrastructure only.
#define CTC_EXACT_MATH_HOST_TABLES
#include "../../ctcdecode_amd/csrc/posterior.h"

namespace {
template <int DT>
int posterior_all(const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank, int log_input, const int32_t *tokens, const int32_t *lens, int R,
                  int L_stride, int32_t *peaks, float *occ, float *conf, float *loglik, int32_t *status) {
  const uint64_t *tbl = ctcmath::host_tables().w;
  std::vector<float> slot(ctcpost::post_slot_bytes(T, L_stride) / 4);  // (sized exactly: a store beyond the slot is a sanitizer report)
  int bad = 0;
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < R; ++r) {
      const size_t h = (size_t)b * R + r, o = h * L_stride;
      const int32_t *y = tokens + o;
      const int rc = log_input == 0 ? ctcpost::posterior_row_host<DT, true>(probs, seq_lens, b, T, V, blank, y, lens[h], L_stride, tbl, slot.data(), peaks + o, occ + o, conf + o, loglik + h)
                                    : ctcpost::posterior_row_host<DT, false>(probs, seq_lens, b, T, V, blank, y, lens[h], L_stride, tbl, slot.data(), peaks + o, occ + o, conf + o, loglik + h);
      if (rc) {
        if (status) status[b] = rc;  // (raised only)
        ++bad;
      }
    }
  return bad;
}
}  // namespace

// probs [B, T, V] of dtype 0 / 1 / 2 (f32 / f16 / bf16); log_input 0 (probabilities) or 1 (log-probabilities; raw logits come as the
// log-softmax rows).  tokens [B, R, L_stride], lens [B, R]; peaks / occ / conf [B, R, L_stride], loglik [B, R], status [B] (raised,
// never cleared) or NULL.  Returns the number of invalid rows, -1 for bad arguments.
extern "C" int ctcpost_host_posteriors(const void *probs, int dtype, const int32_t *seq_lens, int B, int T, int V, int blank, int log_input, const int32_t *tokens,
                                       const int32_t *lens, int R, int L_stride, int32_t *peaks, float *occ, float *conf, float *loglik, int32_t *status) {
  if (B < 0 || T < 0 || V < 1 || R < 0 || L_stride < 0 || blank < 0 || blank >= V || log_input < 0 || log_input > 1 || dtype < 0 || dtype > 2) return -1;
  if ((long long)B * R == 0) return 0;
  if (!lens || !loglik || (L_stride > 0 && (!tokens || !peaks || !occ || !conf)) || (T > 0 && !probs)) return -1;
  if (dtype == ctcskip::kSkipF16) return posterior_all<ctcskip::kSkipF16>(probs, seq_lens, B, T, V, blank, log_input, tokens, lens, R, L_stride, peaks, occ, conf, loglik, status);
  if (dtype == ctcskip::kSkipBF16) return posterior_all<ctcskip::kSkipBF16>(probs, seq_lens, B, T, V, blank, log_input, tokens, lens, R, L_stride, peaks, occ, conf, loglik, status);
  return posterior_all<ctcskip::kSkipF32>(probs, seq_lens, B, T, V, blank, log_input, tokens, lens, R, L_stride, peaks, occ, conf, loglik, status);
}

extern "C" float ctcpost_host_e80(float x) { return ctcpost::e80(x, ctcmath::host_tables().w); }
extern "C" float ctcpost_host_g(float a, float b, float lp, float ll) { return ctcpost::g_step(a, b, lp, ll, ctcmath::host_tables().w); }
extern "C" unsigned long long ctcpost_host_slot_bytes(int T, int L_stride) { return (unsigned long long)ctcpost::post_slot_bytes(T, L_stride); }
extern "C" unsigned long long ctcpost_host_wave_floats(int T) { return (unsigned long long)ctcpost::post_wave_floats(T); }
extern "C" long long ctcpost_host_grid(long long rows, long long budget, unsigned long long slot_bytes) { return ctcpost::post_grid(rows, budget, (size_t)slot_bytes); }
extern "C" long long ctcpost_host_default_scratch() { return ctcpost::kPostDefaultScratch; }
