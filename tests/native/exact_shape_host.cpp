// TEST INFRASTRUCTURE ONLY: the exact-shape policy of the decoder core (ctcdecode_amd/csrc/beam_core.h ShapeExact) on the host.
// Built like core_host.cpp, whose sequential execution policy it reuses by including that file as it is (a library of its own:
// nothing of core_host.cpp's is modified or shared at link time).  One entry point decodes a batch of the twin's shape -- beam 100,
// 29 labels, blank 0, no pruning, no scorer -- with the run-time policy (stage 0: the fixed-layout instantiation the device runs
// today), with the exact policy (stage 1) or with the exact policy that also folds the live beam size (stage 2), and reports the
// event counters of that decode.  With -DCTC_ASSUME_CHECKED every assumption the exact policy hands the optimiser is verified.
#include "core_host.cpp"

namespace {

constexpr int kBeam = 100, kLabels = 29, kBlank = 0;

template <class XT>
int decode_batch(const float *probs, const int32_t *seq_lens, int B, int T, int32_t *out_tokens, int32_t *out_timesteps,
                 float *out_scores, int32_t *out_lens, int32_t *n_results) {
  using namespace ctcbeam;
  const Dims d{kBeam, kLabels, kLabels, 0, 0};
  Work w;
  size_t far_bytes = 0;
  std::vector<char> mem(carve<0>(w, nullptr, nullptr, d, &far_bytes) + 64);
  std::vector<char> far(far_bytes + 64);
  std::vector<PoolNode> pool((size_t)1 + (size_t)kBeam * T);
  std::vector<int> pool_up(2 * pool.size());
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    int len = seq_lens ? seq_lens[b] : T;
    len = std::max(0, std::min(len, T));
    carve<0>(w, mem.data(), far.data(), d, nullptr);
    XT x;
    const OutRefs outs{out_tokens, out_timesteps, out_scores, out_lens, n_results, kBeam, T, nullptr, nullptr, nullptr, nullptr, 0u,
                       nullptr, nullptr, nullptr, nullptr, 0u};
    const int st = decode_utterance<true, 1>(x, w, d, kBlank, probs + (size_t)b * T * kLabels, (const PrunedRows *)nullptr, len, pool.data(),
                                             pool_up.data(), (int)pool.size(), ctcmath::host_tables().w, &outs, b);
    if (st != ST_OK) bad = st;
  }
  return bad ? -bad : 1;
}

}  // namespace

// probs: [B, T, 29] log-probabilities.  events: ctcbeam::EV_COUNT counters of this decode alone (or null).
extern "C" int ctcexact_decode_f32(const float *probs, const int32_t *seq_lens, int B, int T, int stage, int32_t *out_tokens,
                                   int32_t *out_timesteps, float *out_scores, int32_t *out_lens, int32_t *n_results, long long *events) {
  using namespace ctcbeam;
  long long before[EV_COUNT];
  for (int i = 0; i < EV_COUNT; ++i) before[i] = HostX::counters()[i];
  int rc;
  if (stage == 0) rc = decode_batch<HostX>(probs, seq_lens, B, T, out_tokens, out_timesteps, out_scores, out_lens, n_results);
  else if (stage == 1) rc = decode_batch<ShapedX<HostX, ShapeExact<kBeam, kLabels, kBlank, false>>>(probs, seq_lens, B, T, out_tokens, out_timesteps, out_scores, out_lens, n_results);
  else if (stage == 2) rc = decode_batch<ShapedX<HostX, ShapeExact<kBeam, kLabels, kBlank, true>>>(probs, seq_lens, B, T, out_tokens, out_timesteps, out_scores, out_lens, n_results);
  else return -100;
  if (events)
    for (int i = 0; i < EV_COUNT; ++i) events[i] = HostX::counters()[i] - before[i];
  return rc;
}

// the indices of the counters the tests read, so that they need not restate the enum
extern "C" void ctcexact_event_ids(int32_t out[8]) {
  using namespace ctcbeam;
  const int ids[8] = {EV_FRAMES, EV_EXACT, EV_SPEC_OK, EV_SPEC_UNDER, EV_SPEC_OVER, EV_SPEC_OTHER, EV_TIE_FRAMES, EV_COUNT};
  for (int i = 0; i < 8; ++i) out[i] = ids[i];
}
