// keyword_stream.h -- keyword search of live streams (include/ctcdecode_amd.h "Keyword search of live streams"): a stream fed chunk by
// chunk returns, call by call, what keyword.h defines for all frames it was ever fed, bit for bit.  The recurrence of keyword.h runs
// left to right with a free start and a free end, a cell is (value, start frame) and nothing is traced back: what a keyword carries
// from one call to the next is its cells and its best hit so far, and nothing in a cell depends on where a cut falls.
//
// Everything here is CTC_HD code over keyword.h, compiled for both sides: the record a stream keeps in device memory, its size, the
// frame-number rule, and keyword_stream_item_host -- one stream's chunk, sequentially, over the same label_cell / blank_cell / hit_step
// the kernel of keyword_stream.hip runs (the host twin, tests/native/keyword_stream_host.cpp).
#pragma once
#include "keyword.h"

namespace ctckw {

// ---- the record of a stream ----------------------------------------------------------------------------------------------------------
// One block of device memory: [KwStreamHead | KwStreamHit [Q] | KwStreamCell [Q][W]], W = the lane-group width of L_stride.  The kernel
// puts a keyword on a lane group, and lane i of it loads and stores element [q][i] with ONE 16-byte access.
struct KwStreamHead {
  int32_t first;     // F0: added to every frame number
  int32_t frames;    // frames fed so far, written by the call's first block of keywords: for ctcd_keyword_stream_info, never read by a kernel
  int32_t flags;     // kKwEnded
  int32_t Q, L_stride;
  int32_t pad[3];
};
static_assert(sizeof(KwStreamHead) == 32, "the head of a keyword stream's record is 32 bytes");
enum : int { kKwEnded = 1 };
// A keyword's running hit, not yet through hit_final, and the frames the keyword has walked (N).  A call's blocks of keywords run in
// any order and none may read a count another has already advanced: every keyword carries its own.
struct alignas(16) KwStreamHit {
  float v;
  int32_t s, e;
  int32_t frames;
};
static_assert(sizeof(KwStreamHit) == 16, "a keyword's hit is one 16-byte element");
// label i's two cells: d[2i] = a, d[2i + 1] = b
struct alignas(16) KwStreamCell {
  float av;
  int32_t as;
  float bv;
  int32_t bs;
};
static_assert(sizeof(KwStreamCell) == 16, "a label's cells are one 16-byte element");

CTC_HD int kw_stream_width(int L_stride) { return 1 << lane_group_log2(L_stride); }
CTC_HD size_t kw_stream_hits_offset() { return sizeof(KwStreamHead); }
CTC_HD size_t kw_stream_cells_offset(int Q) { return sizeof(KwStreamHead) + (size_t)Q * sizeof(KwStreamHit); }
CTC_HD size_t kw_stream_state_bytes(int Q, int L_stride) {
  return kw_stream_cells_offset(Q) + (size_t)Q * (size_t)kw_stream_width(L_stride) * sizeof(KwStreamCell);
}
CTC_HD KwStreamHit *kw_stream_hits(void *state) { return (KwStreamHit *)((char *)state + kw_stream_hits_offset()); }
CTC_HD KwStreamCell *kw_stream_cells(void *state, int Q) { return (KwStreamCell *)((char *)state + kw_stream_cells_offset(Q)); }

// a fresh record, element by element (keyword_stream_init_kernel spreads the elements over its threads)
CTC_HD KwStreamHead kw_stream_head_init(int first_frame, int Q, int L_stride) {
  KwStreamHead h;
  h.first = first_frame;
  h.frames = h.flags = 0;
  h.Q = Q;
  h.L_stride = L_stride;
  h.pad[0] = h.pad[1] = h.pad[2] = 0;
  return h;
}
CTC_HD KwStreamHit kw_stream_hit_init() {
  KwStreamHit h;
  h.v = neg_inf();
  h.s = h.e = -1;
  h.frames = 0;
  return h;
}
CTC_HD KwStreamCell kw_stream_cell_init() {
  KwStreamCell c;
  c.av = c.bv = neg_inf();
  c.as = c.bs = -1;
  return c;
}

// ---- frame numbers -------------------------------------------------------------------------------------------------------------------
// the rule and the limit of greedy.h's streams: chunk frame t of a stream that had N frames is frame F0 + N + t, at most 2^31 - 1
using ctcgreedy::kStreamMaxFrame;
CTC_HD int kw_stream_frame_no(int first, int frames, int t) { return first + frames + t; }

// what ctcd_last_keyword_kernel reports for a stream call: keyword.h's code of the instantiation, bit 16 set
CTC_HD int kw_stream_kernel_code(int dt, bool prob, bool staged, int lg) { return kw_kernel_code(dt, prob, staged, lg) | (1 << 16); }

// ---- one stream's chunk, sequentially (the host twin) ----------------------------------------------------------------------------------
// Item b of the call's [B, Tc, V] rows, n of its frames; rec: the chunk's frame records (greedy.h frame_recs_host on the rows read
// here); state: the stream's record; kws [Q][L_stride] / lens [Q]: the stream's own list.  sc / st / en and ch_sc / ch_st / ch_en (or
// NULL all three): Q words each; tr_v / tr_s: [Q][Tc] or NULL both; status: Q words, raised to KW_BAD.  Everything is written, the
// record included.
template <int DT, bool PROB>
inline void keyword_stream_item_host(const void *probs, int b, int Tc, int V, int n, int blank, const FrameRec *rec, void *state, const int32_t *kws,
                                     const int32_t *lens, bool eos, float *sc, int32_t *st, int32_t *en, float *tr_v, int32_t *tr_s, float *ch_sc,
                                     int32_t *ch_st, int32_t *ch_en, int32_t *status) {
  KwStreamHead *head = (KwStreamHead *)state;
  const int Q = head->Q, Ls = head->L_stride, W = kw_stream_width(Ls);
  KwStreamHit *hits = kw_stream_hits(state);
  KwStreamCell *cells = kw_stream_cells(state, Q);
  for (int q = 0; q < Q; ++q) {
    const int32_t *kw = kws + (size_t)q * Ls;
    const int len = lens[q];
    float *tv = tr_v ? tr_v + (size_t)q * Tc : nullptr;
    int32_t *ts = tr_v ? tr_s + (size_t)q * Tc : nullptr;
    for (int t = 0; tv && t < Tc; ++t) {
      tv[t] = 0.0f;
      ts[t] = 0;
    }
    bool ok = kw_len_ok(len, Ls);
    for (int i = 0; ok && i < len; ++i) ok = ctcalign::label_ok(kw[i], V, blank);
    Hit run = bad_hit(), chunk = no_hit();
    const int N = hits[q].frames;
    if (ok) {
      const int S = kw_states(len);
      KwStreamCell *mine = cells + (size_t)q * W;
      std::vector<Pair> d((size_t)S), nd((size_t)S);
      for (int s = 0; s < S; ++s) {
        d[(size_t)s].v = (s & 1) ? mine[s >> 1].bv : mine[s >> 1].av;
        d[(size_t)s].s = (s & 1) ? mine[s >> 1].bs : mine[s >> 1].as;
      }
      run.v = hits[q].v;
      run.s = hits[q].s;
      run.e = hits[q].e;
      for (int t = 0; t < n; ++t) {
        const size_t row0 = ((size_t)b * Tc + (size_t)t) * V;
        const int tn = kw_stream_frame_no(head->first, N, t);
        for (int s = 0; s < S; ++s) {
          const int c = (s & 1) ? blank : kw[s >> 1];
          const float r = rel(ctcalign::lp_at<DT, PROB>(probs, row0 + (size_t)c), rec[t].lp);
          if (s & 1) nd[(size_t)s] = blank_cell(r, d[(size_t)s], d[(size_t)s - 1]);
          else nd[(size_t)s] = label_cell(r, d[(size_t)s], s ? d[(size_t)s - 1] : no_path(), s ? d[(size_t)s - 2] : no_path(), s && kw[s >> 1] != kw[(s >> 1) - 1], s == 0, tn);
        }
        d.swap(nd);
        hit_step(run, d[(size_t)S - 1], tn);
        hit_step(chunk, d[(size_t)S - 1], tn);
        if (tv) {
          tv[t] = d[(size_t)S - 1].v;
          ts[t] = d[(size_t)S - 1].s;
        }
      }
      for (int s = 0; s < S; ++s) {
        if (s & 1) {
          mine[s >> 1].bv = d[(size_t)s].v;
          mine[s >> 1].bs = d[(size_t)s].s;
        } else {
          mine[s >> 1].av = d[(size_t)s].v;
          mine[s >> 1].as = d[(size_t)s].s;
        }
      }
      hits[q].v = run.v;
      hits[q].s = run.s;
      hits[q].e = run.e;
      run = hit_final(run);
    } else {
      status[q] = KW_BAD;
      chunk = bad_hit();
    }
    hits[q].frames = N + n;
    sc[q] = run.v;
    st[q] = run.s;
    en[q] = run.e;
    if (ch_sc) {
      chunk = ok ? hit_final(chunk) : chunk;
      ch_sc[q] = chunk.v;
      ch_st[q] = chunk.s;
      ch_en[q] = chunk.e;
    }
  }
  head->frames += n;
  if (eos) head->flags |= kKwEnded;
}

}  // namespace ctckw
