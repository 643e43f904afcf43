// Host twin of the keyword search (ctcdecode_amd/csrc/keyword.h): the routines the kernel of keyword.hip compiles -- the relative
// value, the two cell updates, the walk that picks the window, the validation -- run sequentially, one keyword after the other over
// one item's frame records, behind a C ABI.  Test infrastructure only.
#define CTC_EXACT_MATH_HOST_TABLES
#include "../../ctcdecode_amd/csrc/keyword.h"

#include <type_traits>

namespace {
template <int DT, bool PROB>
void find_all(const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank, const int32_t *kws, const int32_t *lens, int Q, int Ls, float *sc, int32_t *st,
              int32_t *en, float *tv, int32_t *ts, int32_t *status) {
  std::vector<ctcgreedy::FrameRec> rec((size_t)T);
  for (int b = 0; b < B; ++b) {
    const int n = ctcskip::clamped_len(seq_lens, b, T);
    ctcgreedy::frame_recs_host<DT, PROB ? 0 : 1>(probs, b, T, V, n, ctcmath::host_tables().w, rec.data());
    for (int q = 0; q < Q; ++q) {
      const size_t o = (size_t)b * Q + q;
      const int rc = ctckw::keyword_item_host<DT, PROB>(probs, b, T, V, n, blank, rec.data(), kws + (size_t)q * Ls, lens[q], Ls, sc + o, st + o, en + o,
                                                       tv ? tv + o * T : nullptr, ts ? ts + o * T : nullptr);
      if (rc) status[q] = rc;
    }
  }
}
}  // namespace

// probs [B, T, V] of dtype 0 / 1 / 2 (f32 / f16 / bf16); log_input 0 or 1.  kws [Q, Ls], lens [Q]; sc / st / en [B, Q]; tv / ts [B, Q, T]
// or NULL both; status [Q], zeroed by the caller.  Returns 0, -1 for bad arguments.
extern "C" int ctckw_host_find(const void *probs, int dtype, const int32_t *seq_lens, int B, int T, int V, int blank, int log_input, const int32_t *kws,
                               const int32_t *lens, int Q, int Ls, float *sc, int32_t *st, int32_t *en, float *tv, int32_t *ts, int32_t *status) {
  if (B < 0 || T < 0 || V < 1 || Q < 0 || Ls < 0 || Ls > ctckw::kKwMaxLabels || blank < 0 || blank >= V || log_input < 0 || log_input > 1 || dtype < 0 || dtype > 2)
    return -1;
  auto go = [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    if (log_input == 0) find_all<DT, true>(probs, seq_lens, B, T, V, blank, kws, lens, Q, Ls, sc, st, en, tv, ts, status);
    else find_all<DT, false>(probs, seq_lens, B, T, V, blank, kws, lens, Q, Ls, sc, st, en, tv, ts, status);
  };
  if (dtype == ctcskip::kSkipF16) go(std::integral_constant<int, ctcskip::kSkipF16>());
  else if (dtype == ctcskip::kSkipBF16) go(std::integral_constant<int, ctcskip::kSkipBF16>());
  else go(std::integral_constant<int, ctcskip::kSkipF32>());
  return 0;
}
extern "C" int ctckw_host_lane_group(int Ls) { return 1 << ctckw::lane_group_log2(Ls); }
extern "C" int ctckw_host_staged(int V) { return ctckw::kw_staged(V) ? 1 : 0; }
extern "C" int ctckw_host_chunk() { return ctckw::kKwChunk; }
