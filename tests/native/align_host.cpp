// Host twin of the forced alignment (ctcdecode_amd/csrc/align.h): the routines the kernel of align.hip compiles -- cell update, end
// state, back-pointer packing, slot arithmetic, back-trace, row validation -- run sequentially, one hypothesis after the other in one
// scratch slot, behind a C ABI.  Test infrastructure only.
#include "../../ctcdecode_amd/csrc/align.h"

namespace {
template <int DT>
int align_all(const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank, int log_input, const int32_t *tokens, const int32_t *lens, int R,
              int L_stride, int32_t *st, int32_t *en, float *sc, int32_t *status) {
  // exactly one slot, sized by the product's arithmetic: an index that leaves it is a sanitizer report in the stand-alone driver
  std::vector<uint32_t> slot(ctcalign::align_slot_bytes(T, L_stride) / 4);
  int bad = 0;
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < R; ++r) {
      const size_t h = (size_t)b * R + r;
      const int32_t *y = tokens + h * L_stride;
      const int rc = log_input == 0 ? ctcalign::align_row_host<DT, true>(probs, seq_lens, b, T, V, blank, y, lens[h], L_stride, slot.data(), st + h * L_stride,
                                                                         en + h * L_stride, sc + h)
                                    : ctcalign::align_row_host<DT, false>(probs, seq_lens, b, T, V, blank, y, lens[h], L_stride, slot.data(), st + h * L_stride,
                                                                          en + h * L_stride, sc + h);
      if (rc) {
        if (status) status[b] = rc;  // (raised only)
        ++bad;
      }
    }
  return bad;
}
}  // namespace

// probs [B, T, V] of dtype 0 / 1 / 2 (f32 / f16 / bf16); log_input 0 (probabilities) or 1 (log-probabilities; raw logits come as the
// log-softmax rows).  tokens [B, R, L_stride], lens [B, R]; st / en [B, R, L_stride], sc [B, R], status [B] (raised, never cleared) or
// NULL.  Returns the number of invalid rows, -1 for bad arguments.
extern "C" int ctcalign_host_align(const void *probs, int dtype, const int32_t *seq_lens, int B, int T, int V, int blank, int log_input, const int32_t *tokens,
                                   const int32_t *lens, int R, int L_stride, int32_t *st, int32_t *en, float *sc, int32_t *status) {
  if (B < 0 || T < 0 || V < 1 || R < 0 || L_stride < 0 || blank < 0 || blank >= V || log_input < 0 || log_input > 1 || dtype < 0 || dtype > 2) return -1;
  if ((long long)B * R == 0) return 0;
  if (!lens || !sc || (L_stride > 0 && (!tokens || !st || !en)) || (T > 0 && !probs)) return -1;
  if (dtype == ctcskip::kSkipF16) return align_all<ctcskip::kSkipF16>(probs, seq_lens, B, T, V, blank, log_input, tokens, lens, R, L_stride, st, en, sc, status);
  if (dtype == ctcskip::kSkipBF16) return align_all<ctcskip::kSkipBF16>(probs, seq_lens, B, T, V, blank, log_input, tokens, lens, R, L_stride, st, en, sc, status);
  return align_all<ctcskip::kSkipF32>(probs, seq_lens, B, T, V, blank, log_input, tokens, lens, R, L_stride, st, en, sc, status);
}

extern "C" long long ctcalign_host_slot_bytes(int T, int L_stride) { return (long long)ctcalign::align_slot_bytes(T, L_stride); }
extern "C" long long ctcalign_host_grid(long long rows, long long budget, int T, int L_stride) {
  return ctcalign::align_grid(rows, budget, ctcalign::align_slot_bytes(T, L_stride));
}
extern "C" int ctcalign_host_npl(int S) { return ctcalign::align_npl(S); }
extern "C" int ctcalign_host_row_words(int S) { return ctcalign::bp_row_words(S); }
extern "C" int ctcalign_host_max_labels() { return ctcalign::kAlignMaxLabels; }
extern "C" long long ctcalign_host_default_scratch() { return ctcalign::kAlignDefaultScratch; }
