// Host twin of the keyword search of live streams (ctcdecode_amd/csrc/keyword_stream.h): a stream's record in host memory, and one
// chunk call -- keyword_stream_item_host over the chunk's frame records -- behind a C ABI.  Test infrastructure only.
#define CTC_EXACT_MATH_HOST_TABLES
#include "../../ctcdecode_amd/csrc/keyword_stream.h"

#include <stdlib.h>

#include <type_traits>

using namespace ctckw;

// a fresh record for Q keywords of L_stride labels (16-byte aligned); NULL for shapes the library refuses
extern "C" void *ctckws_host_new(int Q, int Ls, long long first_frame) {
  if (Q < 1 || Ls < 1 || Ls > kKwMaxLabels || first_frame < 0 || first_frame > kStreamMaxFrame) return nullptr;
  const size_t bytes = kw_stream_state_bytes(Q, Ls);
  void *state = aligned_alloc(16, (bytes + 15) / 16 * 16);
  *(KwStreamHead *)state = kw_stream_head_init((int)first_frame, Q, Ls);
  for (int q = 0; q < Q; ++q) kw_stream_hits(state)[q] = kw_stream_hit_init();
  for (size_t k = 0; k < (size_t)Q * (size_t)kw_stream_width(Ls); ++k) kw_stream_cells(state, Q)[k] = kw_stream_cell_init();
  return state;
}
extern "C" void ctckws_host_free(void *state) { free(state); }
extern "C" long long ctckws_host_state_bytes(int Q, int Ls) { return (long long)kw_stream_state_bytes(Q, Ls); }
extern "C" int ctckws_host_frames(const void *state) { return ((const KwStreamHead *)state)->frames; }
extern "C" int ctckws_host_ended(const void *state) { return (((const KwStreamHead *)state)->flags & kKwEnded) ? 1 : 0; }

// One chunk for one stream: probs [1, Tc, V] of dtype 0 / 1 / 2, n of its frames; log_input 0 or 1.  kws [Q, Ls], lens [Q]; sc / st /
// en / ch_* [Q]; tv / ts [Q, Tc]; status [Q], zeroed by the caller.  Returns 0, -1 for bad arguments.
extern "C" int ctckws_host_find(void *state, const void *probs, int dtype, int n, int Tc, int V, int blank, int log_input, const int32_t *kws, const int32_t *lens,
                                int eos, float *sc, int32_t *st, int32_t *en, float *tv, int32_t *ts, float *ch_sc, int32_t *ch_st, int32_t *ch_en, int32_t *status) {
  if (!state || Tc < 0 || n < 0 || n > Tc || V < 1 || blank < 0 || blank >= V || log_input < 0 || log_input > 1 || dtype < 0 || dtype > 2) return -1;
  std::vector<ctcgreedy::FrameRec> rec((size_t)Tc);
  auto go = [&](auto dt, auto pr) {
    constexpr int DT = decltype(dt)::value;
    constexpr bool PROB = decltype(pr)::value;
    ctcgreedy::frame_recs_host<DT, PROB ? 0 : 1>(probs, 0, Tc, V, n, ctcmath::host_tables().w, rec.data());
    keyword_stream_item_host<DT, PROB>(probs, 0, Tc, V, n, blank, rec.data(), state, kws, lens, eos != 0, sc, st, en, tv, ts, ch_sc, ch_st, ch_en, status);
  };
  auto mode = [&](auto dt) {
    if (log_input == 0) go(dt, std::true_type());
    else go(dt, std::false_type());
  };
  if (dtype == ctcskip::kSkipF16) mode(std::integral_constant<int, ctcskip::kSkipF16>());
  else if (dtype == ctcskip::kSkipBF16) mode(std::integral_constant<int, ctcskip::kSkipBF16>());
  else mode(std::integral_constant<int, ctcskip::kSkipF32>());
  return 0;
}
