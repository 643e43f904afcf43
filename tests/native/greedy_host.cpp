// Host twin of the greedy decode (ctcdecode_amd/csrc/greedy.h): the routines the kernels of greedy.hip compile -- the argmax step, a
// winner's log-probability in the three input modes, the emit and run-end rules, the run and score bookkeeping, the scratch and shape
// arithmetic -- run sequentially, one item after the other over one set of frame records, behind a C ABI.  Test infrastructure only.
#define CTC_EXACT_MATH_HOST_TABLES
#include "../../ctcdecode_amd/csrc/greedy.h"

#include <vector>

namespace {
template <int DT, int MODE>
void greedy_all(const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank, int32_t *tok, int32_t *st, int32_t *en, float *ls, float *sc,
                int32_t *lens) {
  // exactly one item's records: an index that leaves them is a sanitizer report in the stand-alone driver
  std::vector<ctcgreedy::FrameRec> rec((size_t)T);
  for (int b = 0; b < B; ++b) {
    const size_t o = (size_t)b * T;
    ctcgreedy::greedy_item_host<DT, MODE>(probs, seq_lens, b, T, V, blank, ctcmath::host_tables().w, rec.data(), tok + o, st + o, en ? en + o : nullptr,
                                          ls ? ls + o : nullptr, sc + b, lens + b);
  }
}
template <int DT>
void greedy_mode(int mode, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank, int32_t *tok, int32_t *st, int32_t *en, float *ls,
                 float *sc, int32_t *lens) {
  if (mode == 0) greedy_all<DT, 0>(probs, seq_lens, B, T, V, blank, tok, st, en, ls, sc, lens);
  else if (mode == 1) greedy_all<DT, 1>(probs, seq_lens, B, T, V, blank, tok, st, en, ls, sc, lens);
  else greedy_all<DT, 2>(probs, seq_lens, B, T, V, blank, tok, st, en, ls, sc, lens);
}
}  // namespace

// probs [B, T, V] of dtype 0 / 1 / 2 (f32 / f16 / bf16); log_input 0, 1 or 2.  tok / st / en / ls [B, T] (en, ls may be NULL), sc / lens
// [B].  Returns 0, -1 for bad arguments.
extern "C" int ctcgreedy_host_decode(const void *probs, int dtype, const int32_t *seq_lens, int B, int T, int V, int blank, int log_input, int32_t *tok, int32_t *st,
                                     int32_t *en, float *ls, float *sc, int32_t *lens) {
  if (B < 0 || T < 0 || V < 1 || blank < 0 || blank >= V || log_input < 0 || log_input > 2 || dtype < 0 || dtype > 2) return -1;
  if (B == 0) return 0;
  if (!sc || !lens || (T > 0 && (!probs || !tok || !st))) return -1;
  if (dtype == ctcskip::kSkipF16) greedy_mode<ctcskip::kSkipF16>(log_input, probs, seq_lens, B, T, V, blank, tok, st, en, ls, sc, lens);
  else if (dtype == ctcskip::kSkipBF16) greedy_mode<ctcskip::kSkipBF16>(log_input, probs, seq_lens, B, T, V, blank, tok, st, en, ls, sc, lens);
  else greedy_mode<ctcskip::kSkipF32>(log_input, probs, seq_lens, B, T, V, blank, tok, st, en, ls, sc, lens);
  return 0;
}

// two partial winners combined; -> the index that wins (the arguments' order must not matter)
extern "C" int ctcgreedy_host_combine(float va, int ca, float vb, int cb) {
  ctcgreedy::Winner a, b;
  a.v = va; a.c = ca; b.v = vb; b.c = cb;
  return ctcgreedy::argmax_combine(a, b).c;
}
extern "C" int ctcgreedy_host_lanes_per_frame(int V) { return ctcgreedy::lanes_per_frame(V); }
extern "C" int ctcgreedy_host_vec_rows(unsigned long long base, int V, int dtype, int mode) { return ctcgreedy::vec_rows((uintptr_t)base, V, dtype, mode) ? 1 : 0; }
extern "C" int ctcgreedy_host_logits_f4(int V) { return ctcgreedy::logits_f4(V); }
extern "C" long long ctcgreedy_host_scratch_bytes(long long B, long long T) { return (long long)ctcgreedy::greedy_scratch_bytes(B, T); }
