// stream_peek.h -- interim results of a live stream: what DecoderState::decode() (ctc_beam_search_decoder.cpp:164-211, which
// does not change the state) would return now, read from the PARKED state of the stream (beam_core.h StreamState / save_state)
// without feeding a frame and without writing anything a later chunk reads.  The per-stream routine (peek_stream) is written
// against an execution policy like beam_core.h: the workgroup policy of stream_peek.hip on the GPU, a sequential one on the host
// (tests/native/peek_host.cpp).
//
// Besides the results it reports the length of the longest common prefix of ALL current beam entries.  The beam is a DFS-ordered
// list with an LCP array (Beam::lcp: labels entry j shares with entry j - 1), so that length is min(lcp[1 .. n-1]) -- dep[0] for a
// single entry.  Every entry of a later frame is an entry of this frame or a descendant of one: the common prefix is a prefix of
// everything the stream can still produce, it only grows, and neither its labels nor their time steps change again (a node's time
// step is only updated through a parent that is a beam entry; inside the common prefix no parent is).
#pragma once
#include "beam_core.h"

namespace ctcpeek {

using namespace ctcbeam;

enum : int { PEEK_OK = 0, PEEK_ROW_OVERFLOW = 1 };  // status word of one stream: a reported row does not fit L_cap (nothing of it is written)

// positions of the arrays of a parked state (save_state: arrays[a * K + i])
enum { PA_NODE = 0, PA_CH = 2, PA_DEP = 3, PA_LCP = 4, PA_UP = 8, PA_SCORE = 11, PA_FIN = 13,
       PA_LMST = kStateArrays, PA_LMCL, PA_ACC_LO, PA_ACC_HI, PA_DN, PA_DMLO, PA_DMHI, PA_DFC, PA_SPC_LO, PA_SPC_HI, PA_SPST, PA_SPCL };

struct PeekOut {
  int32_t *tok, *ts;      // [B][n_best][L_cap]
  float *score;           // [B][n_best]
  int32_t *len;           // [B][n_best]
  int32_t *n_results;     // [B]
  int32_t *stable;        // [B]
  int n_best, L_cap;
};

// Scratch of one stream (LDS on the GPU): ONE layout for every beam a stream can have -- 8 bytes per entry for the sort words,
// 8 more with a scorer, ~5.5 for the task lists of the parallel sort.
struct PeekWork {
  uint64_t *pk;          // K: (key48 << 16 | entry), then the reference's result order in the low 16 bits
  float *ext, *approx;   // K each, scorer only: score + last word's LM score | PathTrie::approx_ctc
  int *task;             // 2 x 3 * peek_task_cap(K): pending introsort ranges, by round parity
  int *small;            // 2 * (K / 2 + 1): final ranges (at most 16 elements each)
  int *stack;            // 3 * (2 * 32 + 2): the serial sort of a beam of at most 16 entries
  int *vars;             // PV_COUNT
};
enum { PV_CNT = 0 /* 3 words: sort_parallel's counters */, PV_MIN = 3, PV_OVF = 4, PV_COUNT = 8 };
CTC_HD int peek_task_cap(int K) { return K / 17 + 2; }
CTC_HD size_t peek_carve(PeekWork &w, char *base, int K, bool lm) {
  char *p = base;
  w.pk = carve_ptr<uint64_t>(p, (size_t)K);
  w.ext = carve_ptr<float>(p, lm ? (size_t)K : 0);
  w.approx = carve_ptr<float>(p, lm ? (size_t)K : 0);
  w.task = carve_ptr<int>(p, 6 * (size_t)peek_task_cap(K));
  w.small = carve_ptr<int>(p, 2 * ((size_t)K / 2 + 1));
  w.stack = carve_ptr<int>(p, 3 * (2 * 32 + 2));
  w.vars = carve_ptr<int>(p, PV_COUNT);
  return (size_t)(p - base);
}

CTC_HD double peek_f64(int lo, int hi) {
  union { uint64_t u; double f; } cv;
  cv.u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
  return cv.f;
}

// The scorer state of one beam entry, as save_state parks it (Beam's LM arrays).
struct LmEntry {
  int dep, ch;
  float score;
  uint32_t lmst; int lmcl;
  double acc;
  uint32_t dmlo, dmhi;
  double spc;
  uint32_t spst; int spcl;
};

// decode():168-185 and :194-208 for one prefix under a built-in scorer -- the arithmetic of Decoder::finish(), type for type
// (beam_core.h; a callback scorer's cache may not hold the windows this asks for: its streams are refused on the host side).
CTC_HD void lm_final_scores(const ctclm::LmView &L, const LmEntry &e, float *ext, float *approx) {
  const bool chr = L.char_based != 0;
  const int space = L.space_id;
  // the word the prefix ends in, when it does not end in a space (:173-185; word models only)
  const bool partial = !chr && e.dep > 0 && e.ch != space;
  bool word_here = false;  // a word of the model ends exactly here (path_trie.cpp:59-70: the dictionary allows a space)
  if (partial) {
    if (L.dict_wide) word_here = ctclm::dict_find_wide(L, e.dmlo, e.dmhi, space) >= 0;
    else word_here = space < 32 ? ((e.dmlo >> space) & 1u) != 0u : ((e.dmhi >> (space - 32)) & 1u) != 0u;
  }
  const double wcond = word_here ? e.spc : ctclm::kOovScore;
  float x = e.score;
  if (partial) {
    float score = 0.0f;
    score = (float)(wcond * L.alpha);
    score = (float)((double)score + L.beta);
    x += score;
  }
  *ext = x;
  // Scorer::get_sent_log_prob of the prefix's words (scorer.cpp:95-120): the completed words' windows are summed in acc; then
  // the word it ends in, then "</s>"
  double total = e.acc;
  uint32_t st = e.lmst;
  int cl = e.lmcl;
  if (e.dep == 0) {  // empty prefix: the sentence is N x "<s>" then "</s>" (:97-100)
    total += ctclm::lm_cond(L, &st, &cl, L.w_bos);
  } else if (partial) {
    total += wcond;
    if (word_here) { st = e.spst; cl = e.spcl; }
    else { st = 0u; cl = 0; }  // the word is not in the vocabulary: the window of "</s>" starts behind it
  }
  total += ctclm::lm_cond(L, &st, &cl, L.w_eos);
  double ap = (double)x;
  ap = ap - (double)(size_t)e.dep * L.beta;  // "remove word insert": per label (:203)
  ap -= total * L.alpha;                      // :205
  *approx = (float)ap;
}

// == std::sort(v, v + n, before) of libstdc++, element for element, by the whole workgroup (Decoder::sort_like_std's two routes)
template <class X, class C>
CTC_HD void peek_sort(X &x, const PeekWork &w, int K, uint64_t *v, int n, C before) {
  if (n <= 16) {
    if (x.tid() == 0) stlemu::sort(v, 0, n, before, w.stack);
    x.sync();
    return;
  }
  stlemu::sort_parallel(x, v, n, before, w.task, w.task + 3 * peek_task_cap(K), w.small, w.vars + PV_CNT);
}

// One stream.  hdr / arrays: its parked state; pool, pool_up (express pointers, then the time steps' high parts at pool_up +
// pool_cap): its node pool.  Reports rows [0, min(n_best, #results)) from depth `since` on into row `item` of the outputs; every
// position of that row's buffers this stream does not report is written as zero.  X: tid(), nt(), sync() (a barrier that also
// orders global memory), uni(), atomic_add(), atomic_min(), group() / ngroups() / lane() / lanes().
// Returns PEEK_OK or PEEK_ROW_OVERFLOW (identical in every thread).
template <bool LM, class X>
CTC_HD int peek_stream(X &x, const PeekWork &w, int K, const int *hdr, const int *arrays, const PoolNode *pool, const int *pool_up,
                       int pool_cap, const ctclm::LmView *lm, int since, const PeekOut &o, int item) {
  const int tid = x.tid(), nt = x.nt();
  const int n_best = o.n_best, L_cap = o.L_cap;
  int32_t *out_tok = o.tok + (size_t)item * n_best * L_cap, *out_ts = o.ts + (size_t)item * n_best * L_cap;
  float *out_score = o.score + (size_t)item * n_best;
  int32_t *out_len = o.len + (size_t)item * n_best;
  const int frames = x.uni(hdr[SH_FRAMES]);
  since = since < 0 ? 0 : since;
  if (frames == 0) {
    // no frame yet: the block may be zeroed memory (no init() has run), or parked by empty chunks (no fin order): the result is the
    // root alone, as the one-shot decode of T = 0 gives it
    if (tid == 0) {
      float sc = 0.f;
      if (LM) {
        LmEntry e;
        e.dep = 0; e.ch = -1; e.score = 0.f; e.lmst = lm->s0; e.lmcl = lm->clean0; e.acc = 0.0;
        e.dmlo = 0u; e.dmhi = 0u; e.spc = ctclm::kOovScore; e.spst = 0u; e.spcl = 0;
        float ext;
        lm_final_scores(*lm, e, &ext, &sc);
      }
      out_score[0] = -sc;
      out_len[0] = 0;
      o.n_results[item] = 1;
      o.stable[item] = 0;
    }
    for (int p = 1 + tid; p < n_best; p += nt) { out_score[p] = 0.f; out_len[p] = 0; }
    for (size_t i = (size_t)tid; i < (size_t)n_best * L_cap; i += (size_t)nt) { out_tok[i] = 0; out_ts[i] = 0; }
    return PEEK_OK;
  }
  int n = x.uni(hdr[SH_N]);
  n = n < 1 ? 1 : (n > K ? K : n);  // (1 <= n <= K in every parked state: the scratch is cut for K entries)
  const int *b_node = arrays + (size_t)PA_NODE * K, *b_ch = arrays + (size_t)PA_CH * K, *b_dep = arrays + (size_t)PA_DEP * K;
  const int *b_lcp = arrays + (size_t)PA_LCP * K, *b_up = arrays + (size_t)PA_UP * K, *b_score = arrays + (size_t)PA_SCORE * K;
  const int *fin = arrays + (size_t)PA_FIN * K;  // the order std::nth_element left: where both std::sorts start from
  auto score_of = [&](int a) { return ctcmath::bits_to_f32((uint32_t)b_score[a]); };
  if (tid == 0) { w.vars[PV_MIN] = kIntMax; w.vars[PV_OVF] = 0; }
  if (LM) {
    for (int a = tid; a < n; a += nt) {
      auto A = [&](int arr) { return arrays[(size_t)arr * K + a]; };
      LmEntry e;
      e.dep = b_dep[a]; e.ch = b_ch[a]; e.score = score_of(a);
      e.lmst = (uint32_t)A(PA_LMST); e.lmcl = A(PA_LMCL); e.acc = peek_f64(A(PA_ACC_LO), A(PA_ACC_HI));
      e.dmlo = (uint32_t)A(PA_DMLO); e.dmhi = (uint32_t)A(PA_DMHI);
      e.spc = peek_f64(A(PA_SPC_LO), A(PA_SPC_HI)); e.spst = (uint32_t)A(PA_SPST); e.spcl = A(PA_SPCL);
      lm_final_scores(*lm, e, &w.ext[a], &w.approx[a]);
    }
    x.sync();
  }
  // The two std::sorts (ctc_beam_search_decoder.cpp:188-190, decoder_utils.cpp:59) order by (score desc, character asc); equal
  // float32 scores are common, std::sort is not stable: both are replayed exactly on (key, entry) words, as in finish().
  uint64_t *pk = w.pk;
  for (int p = tid; p < n; p += nt) {
    int a = fin[p];
    a = (unsigned)a < (unsigned)n ? a : p;
    pk[p] = (key48(ord_f32(LM ? w.ext[a] : score_of(a)), mk_info(b_ch[a], 0, 0)) << 16) | (uint64_t)a;
  }
  x.sync();
  auto before = [](uint64_t a, uint64_t c) { return (a >> 16) > (c >> 16); };
  peek_sort(x, w, K, pk, n, before);  // :188-190, by the scores map
  if (LM) {                           // decoder_utils.cpp:59 sorts by the RAW score
    for (int p = tid; p < n; p += nt) {
      const int a = (int)(pk[p] & 0xFFFFu);
      pk[p] = (key48(ord_f32(score_of(a)), mk_info(b_ch[a], 0, 0)) << 16) | (uint64_t)a;
    }
    x.sync();
  }
  peek_sort(x, w, K, pk, n, before);
  // the part of the transcript that is final
  {
    int m = kIntMax;
    for (int j = 1 + tid; j < n; j += nt) m = b_lcp[j] < m ? b_lcp[j] : m;
    if (m != kIntMax) x.atomic_min(&w.vars[PV_MIN], m);
  }
  const int nb = n_best < n ? n_best : n;  // rows reported
  for (int p = tid; p < n_best; p += nt) {
    int j = 0, dj = 0;
    if (p < nb) {
      j = (int)(pk[p] & 0xFFFFu);
      dj = b_dep[j];
      if (dj - since > L_cap) w.vars[PV_OVF] = 1;
    }
    out_score[p] = p < nb ? (LM ? -w.approx[j] : -score_of(j)) : 0.f;  // decoder_utils.cpp:68 (approx_ctc = score without a scorer)
    out_len[p] = dj;
  }
  x.sync();
  const bool ovf = x.uni(w.vars[PV_OVF]) != 0;
  if (tid == 0) {
    const int m = w.vars[PV_MIN];
    o.n_results[item] = nb;
    o.stable[item] = n == 1 ? b_dep[0] : (m < 0 ? 0 : m);
  }
  // path_trie.cpp:113-126 (get_path_vec) for the reported rows, and only for the labels behind depth `since`: segment by segment
  // over the express pointers as in finish() (kExpress) -- segment 0 is the tail above the node's express ancestor, segment
  // i >= 1 the kExpress labels below the i-th express ancestor; one thread per (segment, row), segment-major.  A row's labels
  // of depth <= since are never visited: the loads follow what is reported, not the age of the stream.
  const bool long_t = frames > 65536;  // (frame numbers 0 .. 65535 fit the node's 16 bits)
  const int *pool_thi = pool_up + pool_cap;
  const int nseg = (ovf || frames <= since) ? 0 : (frames - since + kExpress - 1) / kExpress + 1;
  for (int idx = tid; idx < nb * nseg; idx += nt) {
    const int i = idx / nb, p = idx - i * nb;
    const int j = (int)(pk[p] & 0xFFFFu);
    const int dj = b_dep[j];
    const int base = ((dj - 1) / kExpress) * kExpress;  // depth of the first express ancestor
    if (dj <= since || i > base / kExpress) continue;
    int dd = i == 0 ? dj : base - (i - 1) * kExpress;
    int stop = i == 0 ? base : dd - kExpress;
    if (dd <= since) continue;
    stop = stop < since ? since : stop;
    int xn;
    if (i == 0) {
      xn = b_node[j];
    } else {
      xn = b_up[j];
      for (int h = 1; h < i && (unsigned)xn < (unsigned)pool_cap; ++h) xn = pool_up[xn];
    }
    const size_t row = (size_t)p * L_cap;
    while (dd > stop && (unsigned)xn < (unsigned)pool_cap) {  // (a node index outside the pool: a corrupted state is not followed)
      const PoolNode pn = pool[xn];
      out_tok[row + (size_t)(dd - 1 - since)] = pn.ch();
      out_ts[row + (size_t)(dd - 1 - since)] = (int)(pn.cht >> 16) | (long_t ? pool_thi[xn] << 16 : 0);
      xn = pn.parent;
      --dd;
    }
  }
  // positions behind a row's end (and whole rows that report nothing) are zero
  const int grp = x.group(), ngr = x.ngroups(), lane = x.lane(), lanes = x.lanes();
  for (int p = grp; p < n_best; p += ngr) {
    int rep = 0;
    if (p < nb && !ovf) {
      const int dj = b_dep[(int)(pk[p] & 0xFFFFu)];
      rep = dj > since ? dj - since : 0;
    }
    const size_t row = (size_t)p * L_cap;
    for (int q = rep + lane; q < L_cap; q += lanes) { out_tok[row + q] = 0; out_ts[row + q] = 0; }
  }
  return ovf ? PEEK_ROW_OVERFLOW : PEEK_OK;
}

// what the host side asks the translation unit of the kernel for (stream_peek.hip)
struct PeekLaunch {
  char *const *blocks;    // DEVICE [B]: the streams' blocks
  const int *pool_caps;   // DEVICE [B]: nodes their pools hold
  const int *since;       // DEVICE [B]
  long long pool_off;     // byte offset of the node pool inside a block
  int B, K;
  const ctclm::LmView *lm;  // HOST: the scorer's tables as the kernels see them, or null
  PeekOut out;
  int32_t *status;        // DEVICE [B]
};
size_t peek_lds_bytes(int K, bool lm);
int peek_threads(int K);
// queues ctc_stream_peek_kernel on `stream`; returns the hipError_t of the launch as an int
int launch_stream_peek(const PeekLaunch &a, void *stream);
const void *peek_kernel_address(bool lm);

}  // namespace ctcpeek
