// Host twin of the greedy decode of live streams (ctcdecode_amd/csrc/greedy.h "live streams"): the rules greedy_stream.hip's kernel
// compiles -- when the carried run closes, when a run ends or stays open, what the record holds after a chunk -- run sequentially
// (greedy_stream_item_host), one stream after the other over one set of frame records, behind a C ABI.  A stream's state is its
// record, 8 words the caller keeps.  Test infrastructure only.
#define CTC_EXACT_MATH_HOST_TABLES
#include "../../ctcdecode_amd/csrc/greedy.h"

#include <cstring>
#include <vector>

namespace {
template <int DT, int MODE>
void stream_all(ctcgreedy::StreamRec *states, const unsigned char *is_eos, const void *probs, const int32_t *seq_lens, int B, int Tc, int V, int blank, int32_t *tok,
                int32_t *st, int32_t *en, float *ls, int32_t *closed, float *sc, int32_t *lens) {
  // exactly one item's records: an index that leaves them is a sanitizer report in the stand-alone driver
  std::vector<ctcgreedy::FrameRec> rec((size_t)Tc);
  for (int b = 0; b < B; ++b) {
    const size_t o = (size_t)b * Tc, o1 = (size_t)b * (Tc + 1);
    ctcgreedy::greedy_stream_item_host<DT, MODE>(probs, seq_lens, b, Tc, V, blank, ctcmath::host_tables().w, rec.data(), states + b, is_eos[b] != 0, tok + o, st + o,
                                                 en ? en + o1 : nullptr, ls ? ls + o1 : nullptr, sc + b, lens + b, closed ? closed + b : nullptr);
  }
}
template <int DT>
void stream_mode(int mode, ctcgreedy::StreamRec *states, const unsigned char *is_eos, const void *probs, const int32_t *seq_lens, int B, int Tc, int V, int blank,
                 int32_t *tok, int32_t *st, int32_t *en, float *ls, int32_t *closed, float *sc, int32_t *lens) {
  if (mode == 0) stream_all<DT, 0>(states, is_eos, probs, seq_lens, B, Tc, V, blank, tok, st, en, ls, closed, sc, lens);
  else if (mode == 1) stream_all<DT, 1>(states, is_eos, probs, seq_lens, B, Tc, V, blank, tok, st, en, ls, closed, sc, lens);
  else stream_all<DT, 2>(states, is_eos, probs, seq_lens, B, Tc, V, blank, tok, st, en, ls, closed, sc, lens);
}
}  // namespace

extern "C" int ctcgreedy_stream_host_record_bytes() { return (int)sizeof(ctcgreedy::StreamRec); }

// a fresh stream's record into state[0..8)
extern "C" int ctcgreedy_stream_host_init(int32_t *state, long long first_frame) {
  if (!state || first_frame < 0 || first_frame > ctcgreedy::kStreamMaxFrame) return -1;
  const ctcgreedy::StreamRec r = ctcgreedy::stream_rec_init((int)first_frame);
  std::memcpy(state, &r, sizeof r);
  return 0;
}

// {frames fed, emitted, closed, open run 0 / 1, ended 0 / 1}
extern "C" void ctcgreedy_stream_host_info(const int32_t *state, long long out[5]) {
  ctcgreedy::StreamRec r;
  std::memcpy(&r, state, sizeof r);
  out[0] = r.frames;
  out[1] = r.emitted;
  out[2] = r.closed;
  out[3] = ctcgreedy::rec_open(r) ? 1 : 0;
  out[4] = (r.flags & ctcgreedy::kRecEnded) ? 1 : 0;
}

// One chunk call.  states [B][8] words: the streams' records, read and written.  probs [B, Tc, V] of dtype 0 / 1 / 2; tok / st [B, Tc];
// en / ls [B, Tc + 1] and closed [B], or NULL; sc / lens [B].  Returns 0; -1 for bad arguments and for a stream that has ended; -2 for a
// call that would take a stream's frame numbers beyond 2^31 - 1 (here the exact count: the twin knows it).
extern "C" int ctcgreedy_stream_host_decode(int32_t *states, const unsigned char *is_eos, const void *probs, int dtype, const int32_t *seq_lens, int B, int Tc, int V,
                                            int blank, int log_input, int32_t *tok, int32_t *st, int32_t *en, float *ls, int32_t *closed, float *sc, int32_t *lens) {
  if (B < 0 || Tc < 0 || V < 1 || blank < 0 || blank >= V || log_input < 0 || log_input > 2 || dtype < 0 || dtype > 2) return -1;
  if (B == 0) return 0;
  if (!states || !is_eos || !sc || !lens || (Tc > 0 && (!probs || !tok || !st))) return -1;
  std::vector<ctcgreedy::StreamRec> recs((size_t)B);
  std::memcpy(recs.data(), states, (size_t)B * sizeof(ctcgreedy::StreamRec));
  for (int b = 0; b < B; ++b) {
    if (recs[(size_t)b].flags & ctcgreedy::kRecEnded) return -1;
    if ((long long)recs[(size_t)b].first + recs[(size_t)b].frames + Tc > ctcgreedy::kStreamMaxFrame) return -2;
  }
  if (dtype == ctcskip::kSkipF16) stream_mode<ctcskip::kSkipF16>(log_input, recs.data(), is_eos, probs, seq_lens, B, Tc, V, blank, tok, st, en, ls, closed, sc, lens);
  else if (dtype == ctcskip::kSkipBF16) stream_mode<ctcskip::kSkipBF16>(log_input, recs.data(), is_eos, probs, seq_lens, B, Tc, V, blank, tok, st, en, ls, closed, sc, lens);
  else stream_mode<ctcskip::kSkipF32>(log_input, recs.data(), is_eos, probs, seq_lens, B, Tc, V, blank, tok, st, en, ls, closed, sc, lens);
  std::memcpy(states, recs.data(), (size_t)B * sizeof(ctcgreedy::StreamRec));
  return 0;
}
