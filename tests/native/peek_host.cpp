// Host twin of the streaming peek (ctcdecode_amd/csrc/stream_peek.h): one stream of the host build of the core, fed chunk by
// chunk through its parked state, and peek_stream run on that state between chunks under a sequential policy.
// Test infrastructure only.  (The policy, the prune stand-in and the instantiations of the core are core_host.cpp's: that file
// is compiled into this library as it is.)
#include "core_host.cpp"

#include "../../ctcdecode_amd/csrc/stream_peek.h"

namespace {

struct PeekHostX : HostX {
  void atomic_min(int *p, int v) { *p = std::min(*p, v); }
};

struct PeekStream {
  int V = 0, beam = 0, blank = 0, cap_frames = 0, top_n = 0;
  double cutoff_prob = 1.0;
  bool pruned = false;
  ctcbeam::Dims d;
  ctclm::HostScorer hs;
  ctclm::LmView view;
  bool lm = false;
  std::vector<ctcbeam::PoolNode> pool;
  std::vector<int> pool_up, hdr, arrays;
  int frames = 0;
};

}  // namespace

extern "C" void *ctcpeek_host_create(int V, int beam, int cap_frames, double cutoff_prob, int cutoff_top_n, int blank_id, double alpha,
                                     double beta, const char *lm_path, const char *labels) {
  using namespace ctcbeam;
  PeekStream *s = new PeekStream;
  s->V = V; s->beam = beam; s->blank = blank_id; s->cap_frames = cap_frames; s->top_n = cutoff_top_n; s->cutoff_prob = cutoff_prob;
  s->pruned = std::log(cutoff_prob) < 0.0 || cutoff_top_n < V;
  if (lm_path) {
    std::vector<std::string> lab(V);
    for (int i = 0; i < V; ++i) { lab[i] = labels; labels += lab[i].size() + 1; }
    if (!s->hs.build(alpha, beta, lm_path, lab)) { delete s; return nullptr; }
    s->view = s->hs.view();
    s->lm = true;
  }
  s->d.K = beam; s->d.V = V; s->d.Vc_max = s->pruned ? std::min(V, cutoff_top_n) : V; s->d.use_rank_table = s->pruned ? 1 : 0; s->d.lm = s->lm ? 1 : 0;
  s->pool.resize((size_t)1 + (size_t)beam * cap_frames);
  s->pool_up.assign(2 * s->pool.size(), 0);  // express pointers | time steps' high parts
  s->hdr.assign(SH_WORDS, 0);                // a stream that has been fed nothing is a block of zeroed memory
  s->arrays.assign((size_t)kStateArraysLm * beam, 0);
  return s;
}

extern "C" void ctcpeek_host_destroy(void *h) { delete (PeekStream *)h; }

// One chunk of `len` frames ([len, V] log-probabilities); finish != 0 ends the stream and writes its results ([beam, out_T] rows).
extern "C" int ctcpeek_host_feed(void *h, const float *rows, int len, int finish, int32_t *out_tokens, int32_t *out_timesteps,
                                 float *out_scores, int32_t *out_lens, int32_t *n_results, int out_T) {
  using namespace ctcbeam;
  PeekStream &s = *(PeekStream *)h;
  if (s.frames + len > s.cap_frames) return -100;
  const Dims &d = s.d;
  const bool fixed = !s.lm && s.beam <= 128 && s.V <= 32;  // the shapes the device runs with its fixed layout ...
  const Dims cd = fixed ? fixed_layout_dims() : d;         // ... whose workspace is cut for the class, not for the call (decode_kernel.h)
  Work w;
  size_t far_bytes = 0;
  std::vector<char> mem(carve<0>(w, nullptr, nullptr, cd, &far_bytes) + 64, (char)0x5a);  // a fresh workspace every chunk, as a new launch has
  std::vector<char> far(far_bytes + 64, (char)0x5a);
  carve<0>(w, mem.data(), far.data(), cd, nullptr);
  std::vector<int> pcnt(len + 1), pch((size_t)(len + 1) * d.Vc_max);
  std::vector<float> plp((size_t)(len + 1) * d.Vc_max);
  if (s.pruned)
    for (int t = 0; t < len; ++t) prune_row(rows + (size_t)t * s.V, s.V, s.cutoff_prob, s.top_n, &pcnt[t], &pch[(size_t)t * d.Vc_max], &plp[(size_t)t * d.Vc_max]);
  const PrunedRows pr{pcnt.data(), pch.data(), plp.data(), d.Vc_max};
  HostX x;
  StreamState ss{s.hdr.data(), s.arrays.data(), finish ? 1 : 0};
  const OutRefs outs{out_tokens, out_timesteps, out_scores, out_lens, n_results, s.beam, out_T, nullptr, nullptr, nullptr, nullptr, 0u, nullptr, nullptr, nullptr, nullptr, 0u};
  const uint64_t *tbl = ctcmath::host_tables().w;
  const int cap = (int)s.pool.size();
  const PrunedRows *no_pr = nullptr;
  const float *no_rows = nullptr;
  int st;
  if (s.lm) {
    const ctclm::LmView *lm = &s.view;
    const bool word = !lm->char_based && !lm->dict_wide;  // the word-model instantiation, as the product picks it
    if (word && s.pruned) st = decode_utterance<false, false, true, false, false, false, true>(x, w, d, s.blank, no_rows, &pr, len, s.pool.data(), s.pool_up.data(), cap, tbl, &outs, 0, &ss, lm, rows, 1);
    else if (word) st = decode_utterance<true, false, true, false, false, false, true>(x, w, d, s.blank, rows, no_pr, len, s.pool.data(), s.pool_up.data(), cap, tbl, &outs, 0, &ss, lm, rows, 1);
    else if (s.pruned) st = decode_utterance<false, false, true>(x, w, d, s.blank, no_rows, &pr, len, s.pool.data(), s.pool_up.data(), cap, tbl, &outs, 0, &ss, lm, rows, 1);
    else st = decode_utterance<true, false, true>(x, w, d, s.blank, rows, no_pr, len, s.pool.data(), s.pool_up.data(), cap, tbl, &outs, 0, &ss, lm, rows, 1);
  } else if (fixed) {
    if (s.pruned) st = decode_utterance<false, true>(x, w, d, s.blank, no_rows, &pr, len, s.pool.data(), s.pool_up.data(), cap, tbl, &outs, 0, &ss);
    else st = decode_utterance<true, true>(x, w, d, s.blank, rows, no_pr, len, s.pool.data(), s.pool_up.data(), cap, tbl, &outs, 0, &ss);
  } else {
    if (s.pruned) st = decode_utterance<false>(x, w, d, s.blank, no_rows, &pr, len, s.pool.data(), s.pool_up.data(), cap, tbl, &outs, 0, &ss);
    else st = decode_utterance<true>(x, w, d, s.blank, rows, no_pr, len, s.pool.data(), s.pool_up.data(), cap, tbl, &outs, 0, &ss);
  }
  if (st != ST_OK) return -st;
  s.frames += len;
  return 1;
}

// peek_stream on the parked state.  Returns 1, or 0 when a row does not fit L_cap (PEEK_ROW_OVERFLOW).  The state is passed as
// const: `digest` (if not null) receives a checksum of everything a later chunk reads, for "a peek changes nothing".
extern "C" int ctcpeek_host_peek(void *h, int n_best, int since, int32_t *out_tokens, int32_t *out_timesteps, int L_cap, float *out_scores,
                                 int32_t *out_lens, int32_t *n_results, int32_t *stable_len, unsigned long long *digest) {
  using namespace ctcbeam;
  const PeekStream &s = *(const PeekStream *)h;
  ctcpeek::PeekWork w;
  std::vector<char> mem(ctcpeek::peek_carve(w, nullptr, s.beam, s.lm) + 64, (char)0x5a);
  ctcpeek::peek_carve(w, mem.data(), s.beam, s.lm);
  PeekHostX x;
  const ctcpeek::PeekOut o{out_tokens, out_timesteps, out_scores, out_lens, n_results, stable_len, n_best, L_cap};
  const int cap = (int)s.pool.size();
  const int st = s.lm ? ctcpeek::peek_stream<true>(x, w, s.beam, s.hdr.data(), s.arrays.data(), s.pool.data(), s.pool_up.data(), cap, &s.view, since, o, 0)
                      : ctcpeek::peek_stream<false>(x, w, s.beam, s.hdr.data(), s.arrays.data(), s.pool.data(), s.pool_up.data(), cap, (const ctclm::LmView *)nullptr, since, o, 0);
  if (digest) {
    unsigned long long hsh = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t bytes) {
      const unsigned char *c = (const unsigned char *)p;
      for (size_t i = 0; i < bytes; ++i) hsh = (hsh ^ c[i]) * 1099511628211ull;
    };
    mix(s.hdr.data(), s.hdr.size() * 4);
    mix(s.arrays.data(), s.arrays.size() * 4);
    const size_t used = (size_t)s.hdr[SH_POOL];
    for (size_t i = 0; i < used && i < s.pool.size(); ++i) { mix(&s.pool[i].parent, 4); mix(&s.pool[i].lpc, 4); mix(&s.pool[i].cht, 4); }
    mix(s.pool_up.data(), s.pool_up.size() * 4);
    *digest = hsh;
  }
  return st == ctcpeek::PEEK_OK ? 1 : 0;
}

extern "C" int ctcpeek_host_frames(const void *h) { return ((const PeekStream *)h)->frames; }
