// keyword_stream.hip -- keyword search of live streams (include/ctcdecode_amd.h "Keyword search of live streams"): a stream fed chunk
// by chunk returns, call by call, what ctcd_ctc_keywords returns for all its frames together, bit for bit.  What a stream carries
// between calls is keyword_stream.h's record: per keyword the running hit, per label the two cells.  A chunk call queues, on the
// caller's stream and without a host read:
//   one copy of the call's per-stream arguments [record | keywords | lengths | end-of-stream flag] (the decoder's page-locked staging)
//   ctc_keyword_stream_kernel<DT, PROB, STAGED>   a workgroup of four waves per stream and block of keywords; a keyword lies on a lane
//                                                 group of W = 8, 16, 32 or 64 lanes, one label per lane, as in keyword.hip: a frame
//                                                 costs each lane four cross-lane moves (DPP wave_shr:1) and the two cell updates.
//                                                 The group loads its cells at the start and stores them at the end, 16 bytes a lane.
//     STAGED  (V <= 128): ONE launch.  The workgroup stages chunks of F = 32 frames into LDS -- 16-byte loads issued before the chunk
//             in flight is walked, two buffers -- as the raw values; then 8 lanes per frame find the frame's winner there (each lane
//             its columns in increasing index, the 8 partial winners combined by greedy.h's argmax_combine over shuffles), which
//             gives m(t) with the bits of greedy.hip's argmax pass, and the same lanes rewrite their columns in place as r(t, c).
//     gathered (V > 128): greedy.hip's argmax pass in front (two launches), a lane prefetches its own label's values of the next F
//             frames into registers; lane j of a wave loads frame j's blank value and m.
// Raw logits go through the decoder's log-softmax pass first.  Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>
#include <vector>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "keyword_stream.h"

// One keyword stream: the device block [record | keywords | lengths] and what the host knows without reading it.
struct ctcd_keyword_stream {
  int device = 0;
  char *block = nullptr;  // device memory
  size_t kws_off = 0, lens_off = 0;
  int Q = 0, L_stride = 0;
  long long bound = 0;  // F0 + the Tc of every call so far: an upper bound of F0 + the frames fed
  bool ended = false;
  unsigned long long seen_in_call = 0;  // "this stream is already part of the current call"
};

namespace ctckw {

using ctcskip::kSkipBF16;
using ctcskip::kSkipF16;
using ctcskip::kSkipF32;

constexpr int F = kKwChunk;
constexpr int kWinLanes = kKwThreads / F;  // the lanes that share a staged frame's winner
static_assert(kWinLanes == 8, "a staged chunk gives every frame 8 lanes of the workgroup");

// a stream's arguments of one call
struct KwStreamArg {
  void *state;
  const int32_t *kws, *lens;
  int32_t eos, pad;
};
static_assert(sizeof(KwStreamArg) == 32, "a stream's arguments are 32 bytes");

template <int DT> __device__ __forceinline__ float widen_half(uint32_t u16) {
  if (DT == kSkipBF16) return __uint_as_float(u16 << 16);
  return (float)__builtin_bit_cast(_Float16, (uint16_t)u16);
}
template <int DT> __device__ __forceinline__ float elem_at(const void *rows, size_t i) {
  if (DT == kSkipF32) return ((const float *)rows)[i];
  return widen_half<DT>(((const uint16_t *)rows)[i]);
}
template <bool PROB> __device__ __forceinline__ float to_lp(float x) { return PROB ? ctcalign::prob_to_lp(x) : x; }

// the value of the lane to the left (lane - 1 of the wave); lane 0 keeps its own.  DPP wave_shr:1, as in keyword.hip.
__device__ __forceinline__ int left_i(int x) { return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ Pair left_pair(Pair p) {
  Pair q;
  q.v = __int_as_float(left_i(__float_as_int(p.v)));
  q.s = left_i(p.s);
  return q;
}

// a lane's keyword state: its two cells, and on the last label's lane the stream's hit so far and the chunk's
struct StreamLane {
  Pair a, b;  // d[.][2i], d[.][2i + 1]
  Hit h, ch;
  bool first, has2, last;
  float *tr_v;  // the keyword's traces at the chunk's frame 0, or NULL
  int32_t *tr_s;

  // chunk frame `pos`, whose number is tn
  __device__ __forceinline__ void frame(float r_lab, float r_blk, int tn, int pos) {
    const Pair la = left_pair(a), lb = left_pair(b);
    const Pair na = label_cell(r_lab, a, lb, la, has2, first, tn);
    b = blank_cell(r_blk, b, a);
    a = na;
    if (last) {
      hit_step(h, a, tn);
      hit_step(ch, a, tn);
      if (tr_v) {
        tr_v[pos] = a.v;
        tr_s[pos] = a.s;
      }
    }
  }
};

// a fresh record (create, reset)
__global__ void keyword_stream_init_kernel(void *state, int first_frame, int Q, int L_stride) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const size_t cells = (size_t)Q * (size_t)kw_stream_width(L_stride);
  if (i == 0) *(KwStreamHead *)state = kw_stream_head_init(first_frame, Q, L_stride);
  for (size_t k = i; k < (size_t)Q; k += step) kw_stream_hits(state)[k] = kw_stream_hit_init();
  for (size_t k = i; k < cells; k += step) kw_stream_cells(state, Q)[k] = kw_stream_cell_init();
}

// probs [B][T][V]: the chunk; rec: the argmax pass's frame records [B][T] (gathered route only); args [B].  out_sc / out_st / out_en
// [B][Q]; out_tr_v / out_tr_s [B][Q][T] or NULL; out_ch_* [B][Q] or NULL; status [B][Q] or NULL.
template <int DT, bool PROB, bool STAGED>
__global__ void __launch_bounds__(kKwThreads) ctc_keyword_stream_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const FrameRec *rec,
                                                                        const KwStreamArg *args, int Q, int L_stride, int lg, float *out_sc, int32_t *out_st,
                                                                        int32_t *out_en, float *out_tr_v, int32_t *out_tr_s, float *out_ch_sc, int32_t *out_ch_st,
                                                                        int32_t *out_ch_en, int32_t *status) {
  extern __shared__ __attribute__((aligned(16))) float s_r[];  // STAGED: two buffers of F * V values
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, W = 1 << lg, i = lane & (W - 1);
  const int q = (int)blockIdx.y * kw_per_workgroup(lg) + (tid >> lg);
  const int n = ctcskip::clamped_len(seq_lens, b, T);
  const size_t row0 = (size_t)b * T;
  const KwStreamArg A = args[b];
  KwStreamHead *const head = (KwStreamHead *)A.state;
  KwStreamHit *const hits = kw_stream_hits(A.state);
  KwStreamCell *const cells = kw_stream_cells(A.state, Q);
  const int first_frame = head->first;

  // ---- the keyword, from the stream's own list: one label per lane, validated before the first frame
  const bool have = q < Q;
  const int len = have ? A.lens[q] : 0;
  const int lab = have && i < L_stride ? A.kws[(size_t)q * L_stride + i] : blank;
  const bool len_ok = kw_len_ok(len, L_stride), mine = len_ok && i < len;
  const unsigned long long bad_mask = __ballot(have && (!len_ok || (mine && !ctcalign::label_ok(lab, V, blank))));
  const unsigned long long group = (W == 64 ? ~0ull : ((1ull << W) - 1ull)) << (lane & ~(W - 1));
  const bool run = have && (bad_mask & group) == 0ull;
  const int col = run && mine ? lab : blank;  // (always a column of the row)
  const int lab_left = left_i(lab);
  const size_t out = (size_t)b * Q + (size_t)(have ? q : 0);

  // ---- what the stream carried in: the keyword's hit and frame count, the lane's cells (one 16-byte load each)
  const KwStreamHit H = have ? hits[q] : kw_stream_hit_init();
  const KwStreamCell C = run ? cells[(size_t)q * W + i] : kw_stream_cell_init();
  const int tn0 = kw_stream_frame_no(first_frame, H.frames, 0);  // the number of the chunk's frame 0
  StreamLane me;
  me.a.v = C.av;
  me.a.s = C.as;
  me.b.v = C.bv;
  me.b.s = C.bs;
  me.h.v = H.v;
  me.h.s = H.s;
  me.h.e = H.e;
  me.ch = no_hit();
  me.first = i == 0;
  me.has2 = i > 0 && lab != lab_left;
  me.last = run && i == len - 1;
  me.tr_v = out_tr_v ? out_tr_v + out * T : nullptr;
  me.tr_s = out_tr_v ? out_tr_s + out * T : nullptr;

  if (STAGED) {
    // A chunk: the frames [t0, t0 + fr) of the item, cnt = fr * V consecutive elements of the input.  Those of them that make up whole
    // aligned 16-byte words are loaded as such (up to four words a thread), the few in front and behind one by one.
    constexpr int kElems = DT == kSkipF32 ? 4 : 8, kBytes = DT == kSkipF32 ? 4 : 2, kVecs = 4;
    uint4 vq[kVecs];
    uint32_t edge = 0u;
    int head_n = 0, nvec = 0, tail = 0;
    auto prefetch = [&](int t0) {
      const int fr = n - t0 < F ? n - t0 : F, cnt = fr * V;
      const char *p = (const char *)probs + (row0 + (size_t)t0) * (size_t)V * kBytes;
      head_n = (int)((0u - (unsigned)(uintptr_t)p) & 15u) / kBytes;
      head_n = head_n < cnt ? head_n : cnt;
      nvec = (cnt - head_n) / kElems;
      tail = cnt - head_n - nvec * kElems;
      const uint4 *pv = reinterpret_cast<const uint4 *>(p + (size_t)head_n * kBytes);
#pragma unroll
      for (int u = 0; u < kVecs; ++u) {
        const int iv = tid + kKwThreads * u;
        if (iv < nvec) vq[u] = pv[iv];
      }
      int e = -1;
      if (tid < head_n) e = tid;
      else if (tid >= 64 && tid - 64 < tail) e = head_n + nvec * kElems + (tid - 64);
      if (e >= 0) edge = DT == kSkipF32 ? ((const uint32_t *)p)[e] : (uint32_t)((const uint16_t *)p)[e];
    };
    auto put = [&](float *dst, int j, uint32_t raw) { dst[j] = DT == kSkipF32 ? __uint_as_float(raw) : widen_half<DT>(raw); };
    auto store_raw = [&](float *dst) {  // the prefetched chunk into LDS, widened, as it was read
#pragma unroll
      for (int u = 0; u < kVecs; ++u) {
        const int iv = tid + kKwThreads * u;
        if (iv < nvec) {
          const int j = head_n + iv * kElems;
          const uint32_t w[4] = {vq[u].x, vq[u].y, vq[u].z, vq[u].w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (DT == kSkipF32) {
              put(dst, j + k, w[k]);
            } else {
              put(dst, j + 2 * k, w[k] & 0xffffu);
              put(dst, j + 2 * k + 1, w[k] >> 16);
            }
          }
        }
      }
      if (tid < head_n) put(dst, tid, edge);
      else if (tid >= 64 && tid - 64 < tail) put(dst, head_n + nvec * kElems + (tid - 64), edge);
    };
    // The frame's winner and the relative values, in place.  Lane `sub` of the 8 that share frame f owns the columns sub, sub + 8, ...:
    // it walks them in increasing index (argmax_step), the 8 partial winners of disjoint columns meet in a butterfly (argmax_combine:
    // the greater value, else the smaller index), and every lane has the winner greedy.hip's argmax pass finds -- the first index of
    // the greatest value, with that element's bits.  Each lane then rewrites the columns it has read, so no barrier lies in between.
    auto settle = [&](float *dst, int fr) {
      const int f = tid / kWinLanes, sub = tid % kWinLanes;
      float *row = dst + f * V;
      ctcgreedy::Winner w = ctcgreedy::no_winner();
      if (f < fr)
        for (int c = sub; c < V; c += kWinLanes) ctcgreedy::argmax_step(w, row[c], c);
#pragma unroll
      for (int off = 1; off < kWinLanes; off <<= 1) {
        ctcgreedy::Winner o;
        o.v = __shfl_xor(w.v, off, 64);
        o.c = __shfl_xor(w.c, off, 64);
        w = ctcgreedy::argmax_combine(w, o);
      }
      const float m = ctcgreedy::winner_lp<PROB ? ctcgreedy::kModeProb : ctcgreedy::kModeLog>(w.v);
      if (f < fr)
        for (int c = sub; c < V; c += kWinLanes) row[c] = rel(to_lp<PROB>(row[c]), m);
    };
    const int chunk = F * V;
    if (n > 0) {
      prefetch(0);
      store_raw(s_r);
      __syncthreads();
      settle(s_r, n < F ? n : F);
      __syncthreads();
    }
    int buf = 0;
    for (int t0 = 0; t0 < n; t0 += F) {
      const bool more = t0 + F < n;
      if (more) prefetch(t0 + F);  // (in flight while this chunk is walked)
      const float *cur = s_r + buf * chunk;
      const int fr = n - t0 < F ? n - t0 : F;
      if (fr == F) {  // (a whole chunk: unrolled, so that the LDS reads of the frames ahead are issued early)
#pragma unroll 8
        for (int j = 0; j < F; ++j) me.frame(cur[j * V + col], cur[j * V + blank], tn0 + t0 + j, t0 + j);
      } else {
        for (int j = 0; j < fr; ++j) me.frame(cur[j * V + col], cur[j * V + blank], tn0 + t0 + j, t0 + j);
      }
      if (more) {
        float *nxt = s_r + (buf ^ 1) * chunk;
        store_raw(nxt);
        __syncthreads();
        settle(nxt, n - (t0 + F) < F ? n - (t0 + F) : F);
      }
      __syncthreads();  // (the other buffer is complete; this one is free)
      buf ^= 1;
    }
  } else {
    // A chunk in registers: the lane's own label at each of the F frames, and -- lane j for frame j -- the blank's value and m.
    float nl[F], nb = 0.0f, nm = 0.0f, cl[F], cb = 0.0f;
    auto prefetch = [&](int t0) {
#pragma unroll
      for (int j = 0; j < F; ++j) nl[j] = t0 + j < n ? elem_at<DT>(probs, (row0 + (size_t)(t0 + j)) * V + (size_t)col) : 0.0f;
      const int t = t0 + (lane & (F - 1));
      if (t < n) {
        nb = elem_at<DT>(probs, (row0 + (size_t)t) * V + (size_t)blank);
        nm = rec[row0 + (size_t)t].lp;
      }
    };
    if (n > 0) prefetch(0);
    for (int t0 = 0; t0 < n; t0 += F) {
      cb = rel(to_lp<PROB>(nb), nm);
#pragma unroll
      for (int j = 0; j < F; ++j) cl[j] = rel(to_lp<PROB>(nl[j]), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nm), j)));
      if (t0 + F < n) prefetch(t0 + F);  // (in flight while this chunk is walked)
#pragma unroll
      for (int j = 0; j < F; ++j)
        if (t0 + j < n) me.frame(cl[j], __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cb), j)), tn0 + t0 + j, t0 + j);
    }
  }

  // ---- the results, on the last label's lane; an invalid keyword's on the group's first
  if (me.last || (have && !run && i == 0)) {
    const Hit h = run ? hit_final(me.h) : bad_hit();
    out_sc[out] = h.v;
    out_st[out] = h.s;
    out_en[out] = h.e;
    if (out_ch_sc) {
      const Hit c = run ? hit_final(me.ch) : bad_hit();
      out_ch_sc[out] = c.v;
      out_ch_st[out] = c.s;
      out_ch_en[out] = c.e;
    }
    if (!run && status) status[out] = KW_BAD;
  }
  // the traces at and beyond n (an invalid keyword's: everywhere) are 0
  if (have && me.tr_v)
    for (int t = (run ? n : 0) + i; t < T; t += W) {
      me.tr_v[t] = 0.0f;
      me.tr_s[t] = 0;
    }
  // ---- what the stream carries on: the group's cells (one 16-byte store a lane), the hit, the keyword's frame count
  if (run) {
    KwStreamCell c;
    c.av = me.a.v;
    c.as = me.a.s;
    c.bv = me.b.v;
    c.bs = me.b.s;
    cells[(size_t)q * W + i] = c;
  }
  if (me.last) {
    hits[q].v = me.h.v;
    hits[q].s = me.h.s;
    hits[q].e = me.h.e;
  }
  if (have && i == 0) hits[q].frames = H.frames + n;
  if (blockIdx.y == 0 && tid == 0) {  // (no kernel reads these two words)
    head->frames += n;
    if (A.eos) head->flags |= kKwEnded;
  }
}

template <int DT, bool PROB, bool STAGED, typename... Args> void stream_launch_one(dim3 grid, size_t lds, hipStream_t s, Args... args) {
  hipLaunchKernelGGL((ctc_keyword_stream_kernel<DT, PROB, STAGED>), grid, dim3(kKwThreads), lds, s, args...);
}
template <int DT, typename... Args> void stream_launch_dt(bool prob, bool staged, dim3 grid, size_t lds, hipStream_t s, Args... args) {
  if (prob && staged) stream_launch_one<DT, true, true>(grid, lds, s, args...);
  else if (prob) stream_launch_one<DT, true, false>(grid, lds, s, args...);
  else if (staged) stream_launch_one<DT, false, true>(grid, lds, s, args...);
  else stream_launch_one<DT, false, false>(grid, lds, s, args...);
}

std::atomic<unsigned long long> g_kw_stream_calls{0};

int kw_first_frame_ok(long long first_frame, const std::string &f) {
  if (first_frame < 0 || first_frame > kStreamMaxFrame) return ctcalign::align_fail(CTCD_EINVAL, (f + "0 <= first_frame <= 2^31 - 1 required").c_str());
  return CTCD_OK;
}
int kw_hip_fail(const std::string &what, hipError_t e) { return ctcalign::align_fail(CTCD_EHIP, (what + ": " + hipGetErrorString(e)).c_str()); }
void launch_init(const ctcd_keyword_stream *st, long long first_frame, hipStream_t s) {
  const long long cells = (long long)st->Q * kw_stream_width(st->L_stride);
  const long long blocks = (cells + 255) / 256;
  hipLaunchKernelGGL(keyword_stream_init_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks))), dim3(256), 0, s, (void *)st->block,
                     (int)first_frame, st->Q, st->L_stride);
}

}  // namespace ctckw

using namespace ctckw;
using ctcalign::align_fail;

extern "C" {

int ctcd_keyword_stream_create(ctcd_decoder *d, ctcd_keyword_stream **out, const int32_t *keywords, const int32_t *keyword_lens, int Q, int L_stride,
                               long long first_frame) {
  const std::string f = "ctcd_keyword_stream_create: ";
  if (!d || !out) return align_fail(CTCD_EINVAL, (f + "decoder == NULL or out == NULL").c_str());
  *out = nullptr;
  if (Q < 1 || L_stride < 1 || !keywords || !keyword_lens) return align_fail(CTCD_EINVAL, (f + "Q >= 1, L_stride >= 1 and both keyword tensors required").c_str());
  if (L_stride > kKwMaxLabels) return align_fail(CTCD_EUNSUPPORTED, (f + "keywords of more than 64 labels (L_stride > 64) are not built").c_str());
  const int per_wg = kw_per_workgroup(lane_group_log2(L_stride));
  if (((long long)Q + per_wg - 1) / per_wg > 65535) return align_fail(CTCD_EUNSUPPORTED, (f + "too many keywords for one launch").c_str());
  if (const int rc = kw_first_frame_ok(first_frame, f)) return rc;
  ctcalign::AlignDecoderInfo inf;
  if (const int rc = ctcalign::align_decoder_info(d, &inf)) return rc;
  ctcdev::DeviceGuard guard;
  if (guard.enter(inf.device) != hipSuccess) return kw_hip_fail("hipSetDevice", guard.err);
  ctcd_keyword_stream *st = new ctcd_keyword_stream();
  st->device = inf.device;
  st->Q = Q;
  st->L_stride = L_stride;
  st->bound = first_frame;
  st->kws_off = (kw_stream_state_bytes(Q, L_stride) + 255) & ~(size_t)255;
  st->lens_off = st->kws_off + (size_t)Q * L_stride * sizeof(int32_t);
  hipError_t e = hipMalloc((void **)&st->block, st->lens_off + (size_t)Q * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemcpy(st->block + st->kws_off, keywords, (size_t)Q * L_stride * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(st->block + st->lens_off, keyword_lens, (size_t)Q * sizeof(int32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    // (the record is in place when the call returns: the stream's first chunk may be queued on any stream)
    launch_init(st, first_frame, nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  }
  if (e != hipSuccess) {
    if (st->block) (void)hipFree(st->block);
    delete st;
    return kw_hip_fail(f + "the stream's record", e);
  }
  *out = st;
  return CTCD_OK;
}

void ctcd_keyword_stream_destroy(ctcd_decoder *d, ctcd_keyword_stream *st) {
  (void)d;
  if (!st) return;
  ctcdev::DeviceGuard guard;
  if (guard.enter(st->device) == hipSuccess && st->block) (void)hipFree(st->block);
  delete st;
}

int ctcd_keyword_stream_reset(ctcd_decoder *d, ctcd_keyword_stream *st, long long first_frame, void *stream) {
  const std::string f = "ctcd_keyword_stream_reset: ";
  if (!d || !st) return align_fail(CTCD_EINVAL, (f + "decoder == NULL or stream state == NULL").c_str());
  if (const int rc = kw_first_frame_ok(first_frame, f)) return rc;
  ctcdev::DeviceGuard guard;
  if (guard.enter(st->device) != hipSuccess) return kw_hip_fail("hipSetDevice", guard.err);
  launch_init(st, first_frame, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return kw_hip_fail(f + "the stream's record", e);
  st->bound = first_frame;
  st->ended = false;
  return CTCD_OK;
}

int ctcd_keyword_stream_find(ctcd_decoder *d, ctcd_keyword_stream **states, const unsigned char *is_eos, const void *probs, const int32_t *seq_lens, int B, int Tc,
                             int V, int blank_id, int log_input, float *out_scores, int32_t *out_starts, int32_t *out_ends, float *out_end_scores,
                             int32_t *out_end_starts, float *out_chunk_scores, int32_t *out_chunk_starts, int32_t *out_chunk_ends, int32_t *status, void *stream) {
  const std::string f = "ctcd_keyword_stream_find: ";
  if (!d) return align_fail(CTCD_EINVAL, "decoder == NULL");
  if (B < 0 || Tc < 0 || V < 1) return align_fail(CTCD_EINVAL, (f + "B, Tc >= 0 and V >= 1 required").c_str());
  if (blank_id < 0 || blank_id >= V) return align_fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (log_input < 0 || log_input > 2) return align_fail(CTCD_EINVAL, (f + "log_input must be 0, 1 or 2").c_str());
  if (B == 0) return CTCD_OK;
  const bool details = out_chunk_scores != nullptr;
  if (!states || !is_eos || !out_scores || !out_starts || !out_ends || (Tc > 0 && !probs) || (details && (!out_chunk_starts || !out_chunk_ends)) ||
      (!details && (out_chunk_starts || out_chunk_ends || out_end_scores || out_end_starts)) || (details && Tc > 0 && (!out_end_scores || !out_end_starts)))
    return align_fail(CTCD_EINVAL, (f + "null tensor (the traces and the chunk results come together)").c_str());
  if (V > (1 << 28)) return align_fail(CTCD_EUNSUPPORTED, (f + "V > 2^28").c_str());
  ctcalign::AlignDecoderInfo inf;
  if (const int rc = ctcalign::align_decoder_info(d, &inf)) return rc;
  const unsigned long long call = ++g_kw_stream_calls;
  for (int b = 0; b < B; ++b) {
    ctcd_keyword_stream *st = states[b];
    if (!st) return align_fail(CTCD_EINVAL, (f + "a stream state is NULL").c_str());
    if (st->device != inf.device) return align_fail(CTCD_EINVAL, (f + "a stream state lives on another device than the decoder").c_str());
    if (st->ended) return align_fail(CTCD_EINVAL, (f + "a stream has ended: reset it before it is fed again").c_str());
    if (st->seen_in_call == call) return align_fail(CTCD_EINVAL, (f + "the same stream twice in one call").c_str());
    if (st->Q != states[0]->Q || st->L_stride != states[0]->L_stride)
      return align_fail(CTCD_EINVAL, (f + "the streams of one call must share Q and L_stride").c_str());
    st->seen_in_call = call;
  }
  for (int b = 0; b < B; ++b)
    if (states[b]->bound + Tc > kStreamMaxFrame) return align_fail(CTCD_EUNSUPPORTED, (f + "a stream's frame numbers would pass 2^31 - 1").c_str());
  const int Q = states[0]->Q, L_stride = states[0]->L_stride;
  const int lg = lane_group_log2(L_stride), per_wg = kw_per_workgroup(lg);
  const long long blocks = ((long long)Q + per_wg - 1) / per_wg;  // (<= 65535: checked at create)
  ctcdev::DeviceGuard guard;
  if (guard.enter(inf.device) != hipSuccess) return kw_hip_fail("hipSetDevice", guard.err);
  hipStream_t s = (hipStream_t)stream;
  std::vector<KwStreamArg> args((size_t)B);
  for (int b = 0; b < B; ++b) {
    const ctcd_keyword_stream *st = states[b];
    args[(size_t)b].state = st->block;
    args[(size_t)b].kws = (const int32_t *)(st->block + st->kws_off);
    args[(size_t)b].lens = (const int32_t *)(st->block + st->lens_off);
    args[(size_t)b].eos = is_eos[b] ? 1 : 0;
    args[(size_t)b].pad = 0;
  }
  int dtype = inf.in_dtype;
  if (log_input == 2 && Tc > 0) {  // raw logits: the log-softmax pass into the decoder's float32 rows, then log-probabilities
    const float *rows32 = nullptr;
    if (const int rc = ctcalign::align_lsm_rows(d, probs, seq_lens, B, Tc, V, stream, &rows32)) return rc;
    probs = rows32;
    dtype = CTCD_DTYPE_F32;
  }
  const bool prob = log_input == 0, staged = kw_staged(V);
  void *rec = nullptr, *dargs = nullptr;
  if (!staged && Tc > 0)
    if (const int rc = ctcgreedy::greedy_scratch(d, ctcgreedy::greedy_scratch_bytes(B, Tc), &rec)) return rc;
  if (const int rc = ctcgreedy::greedy_stream_upload(d, args.data(), args.size() * sizeof(KwStreamArg), stream, &dargs)) return rc;
  if (rec) {
    ctcgreedy::launch_argmax_pass(dtype, prob ? ctcgreedy::kModeProb : ctcgreedy::kModeLog, probs, seq_lens, (long long)B * Tc, Tc, V, (FrameRec *)rec, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return kw_hip_fail("keyword stream argmax", e);
  }
  const dim3 grid((unsigned)B, (unsigned)blocks);
  const size_t lds = kw_lds_bytes(V);
  const int dt = dtype == CTCD_DTYPE_F16 ? kSkipF16 : (dtype == CTCD_DTYPE_BF16 ? kSkipBF16 : kSkipF32);
  auto go = [&](auto tag) {
    stream_launch_dt<decltype(tag)::value>(prob, staged, grid, lds, s, probs, seq_lens, Tc, V, blank_id, (const FrameRec *)rec, (const KwStreamArg *)dargs, Q,
                                           L_stride, lg, out_scores, out_starts, out_ends, Tc > 0 ? out_end_scores : nullptr, Tc > 0 ? out_end_starts : nullptr,
                                           out_chunk_scores, out_chunk_starts, out_chunk_ends, status);
  };
  if (dt == kSkipF16) go(std::integral_constant<int, kSkipF16>());
  else if (dt == kSkipBF16) go(std::integral_constant<int, kSkipBF16>());
  else go(std::integral_constant<int, kSkipF32>());
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return kw_hip_fail("keyword stream search", e);
  keyword_note_kernel(d, kw_stream_kernel_code(dt, prob, staged, lg));
  for (int b = 0; b < B; ++b) {
    states[b]->bound += Tc;
    if (is_eos[b]) states[b]->ended = true;
  }
  return CTCD_OK;
}

int ctcd_keyword_stream_info(ctcd_decoder *d, const ctcd_keyword_stream *st, long long out[4]) {
  const std::string f = "ctcd_keyword_stream_info: ";
  if (!d || !st || !out) return align_fail(CTCD_EINVAL, (f + "decoder, stream state and out required").c_str());
  ctcdev::DeviceGuard guard;
  if (guard.enter(st->device) != hipSuccess) return kw_hip_fail("hipSetDevice", guard.err);
  hipError_t e = hipDeviceSynchronize();  // (whatever stream the stream's calls were queued on)
  KwStreamHead h;
  if (e == hipSuccess) e = hipMemcpy(&h, st->block, sizeof h, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return kw_hip_fail(f + "the stream's record", e);
  out[0] = h.frames;
  out[1] = h.Q;
  out[2] = h.L_stride;
  out[3] = (h.flags & kKwEnded) ? 1 : 0;
  return CTCD_OK;
}

}  // extern "C"
