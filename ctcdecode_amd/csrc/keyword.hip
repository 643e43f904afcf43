// keyword.hip -- keyword search of keyword.h on the device, and its C ABI (include/ctcdecode_amd.h "Keyword search").  A translation
// unit of its own, like align.hip and greedy.hip: no kernel of ctcdecode_amd.hip or decode_kernels.hip sees it.  Two launches queued
// behind each other on the caller's stream (behind the log-softmax pass for raw logits), nothing read on the host in between:
//   greedy.hip's argmax pass, unchanged: m(t) = lp(t, c*(t)) of every frame into the decoder's frame records
//   ctc_keyword_kernel<DT, PROB, STAGED>   a workgroup of four waves per item and block of keywords; all four waves walk the same
//                                          frames.  A keyword lies on a lane group of W = 8, 16, 32 or 64 lanes (a runtime width), one
//                                          label per lane: the label state 2i and the blank state 2i + 1 behind it are two (value,
//                                          start) pairs in lane i's registers, and a frame costs each lane four cross-lane moves from
//                                          its left neighbour (DPP wave_shr:1; the first lane of a group ignores what it gets), the
//                                          two cell updates of keyword.h, and on the last label's lane the `>=` walk of the result.
//     STAGED  (V <= 128): the workgroup stages chunks of F = 32 frames into LDS as r(t, c) -- 16-byte loads issued before the chunk
//             in flight is walked, converted (the binary64 log of probabilities once per element per workgroup) and written behind
//             it, two buffers -- and a lane reads its label's and the blank's column from LDS.
//     gathered (V > 128): a lane prefetches its own label's values of the next F frames into registers, F loads in flight; lane j of
//             a wave loads frame j's blank value and m, and the frame's turn takes them by readlane.
// Nothing is loaded from HBM on a frame's critical path.  Every store is a plain C++ store; there is no inline assembly.
// With ctcd_set_long_keywords on, a call of 65 <= L_stride <= 2048 goes to keyword_long.hip's kernel behind the same argmax pass.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "keyword.h"
#include "keyword_long.h"

namespace ctckw {

using ctcskip::kSkipBF16;
using ctcskip::kSkipF16;
using ctcskip::kSkipF32;

constexpr int F = kKwChunk;

template <int DT> __device__ __forceinline__ float widen_half(uint32_t u16) {
  if (DT == kSkipBF16) return __uint_as_float(u16 << 16);
  return (float)__builtin_bit_cast(_Float16, (uint16_t)u16);
}
template <int DT> __device__ __forceinline__ float elem_at(const void *rows, size_t i) {
  if (DT == kSkipF32) return ((const float *)rows)[i];
  return widen_half<DT>(((const uint16_t *)rows)[i]);
}
template <bool PROB> __device__ __forceinline__ float to_lp(float x) { return PROB ? ctcalign::prob_to_lp(x) : x; }

// the value of the lane to the left (lane - 1 of the wave); lane 0 keeps its own.  DPP wave_shr:1: one v_mov, no LDS crossbar.
__device__ __forceinline__ int left_i(int x) {
#ifdef CTC_KW_SHFL
  return __shfl_up(x, 1, 64);
#else
  return __builtin_amdgcn_update_dpp(x, x, 0x138, 0xf, 0xf, false);
#endif
}
__device__ __forceinline__ Pair left_pair(Pair p) {
  Pair q;
  q.v = __int_as_float(left_i(__float_as_int(p.v)));
  q.s = left_i(p.s);
  return q;
}

// a lane's keyword state: its two cells, and on the last label's lane the result so far
struct Lane {
  Pair a, b;  // d[.][2i], d[.][2i + 1]
  Hit h;
  bool first, has2, last;
  float *tr_v;  // the keyword's traces at frame 0, or NULL
  int32_t *tr_s;

  __device__ __forceinline__ void frame(float r_lab, float r_blk, int t) {
    const Pair la = left_pair(a), lb = left_pair(b);
    const Pair na = label_cell(r_lab, a, lb, la, has2, first, t);
    b = blank_cell(r_blk, b, a);
    a = na;
    if (last) {
      hit_step(h, a, t);
      if (tr_v) {
        tr_v[t] = a.v;
        tr_s[t] = a.s;
      }
    }
  }
};

template <int DT, bool PROB, bool STAGED>
__global__ void __launch_bounds__(kKwThreads) ctc_keyword_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const FrameRec *rec,
                                                                 const int32_t *keywords, const int32_t *keyword_lens, int Q, int L_stride, int lg, float *out_sc,
                                                                 int32_t *out_st, int32_t *out_en, float *out_tr_v, int32_t *out_tr_s, int32_t *status) {
  extern __shared__ __attribute__((aligned(16))) float s_r[];  // STAGED: two buffers of F * V values r(t, c)
  __shared__ float s_m[F];                                     // STAGED: m(t) of the chunk being converted
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, W = 1 << lg, i = lane & (W - 1);
  const int q = (int)blockIdx.y * kw_per_workgroup(lg) + (tid >> lg);
  const int n = ctcskip::clamped_len(seq_lens, b, T);
  const size_t row0 = (size_t)b * T;

  // ---- the keyword: one label per lane, validated before the first frame
  const bool have = q < Q;
  const int len = have ? keyword_lens[q] : 0;
  const int lab = have && i < L_stride ? keywords[(size_t)q * L_stride + i] : blank;
  const bool len_ok = kw_len_ok(len, L_stride), mine = len_ok && i < len;
  const unsigned long long bad_mask = __ballot(have && (!len_ok || (mine && !ctcalign::label_ok(lab, V, blank))));
  const unsigned long long group = (W == 64 ? ~0ull : ((1ull << W) - 1ull)) << (lane & ~(W - 1));
  const bool run = have && (bad_mask & group) == 0ull;
  const int col = run && mine ? lab : blank;  // (always a column of the row)
  const int lab_left = left_i(lab);
  const size_t out = (size_t)b * Q + (size_t)(have ? q : 0);
  Lane me;
  me.a = me.b = no_path();
  me.h = no_hit();
  me.first = i == 0;
  me.has2 = i > 0 && lab != lab_left;
  me.last = run && i == len - 1;
  me.tr_v = out_tr_v ? out_tr_v + out * T : nullptr;
  me.tr_s = out_tr_v ? out_tr_s + out * T : nullptr;

  if (STAGED) {
    // A chunk: the frames [t0, t0 + fr) of the item, cnt = fr * V consecutive elements from element e0 of the input.  Those of them that
    // make up whole aligned 16-byte words are loaded as such (up to four words a thread), the few in front and behind one by one.
    constexpr int kElems = DT == kSkipF32 ? 4 : 8, kBytes = DT == kSkipF32 ? 4 : 2, kVecs = 4;
    uint4 vq[kVecs];
    uint32_t edge = 0u;
    float m_next = 0.0f;
    int head = 0, nvec = 0, tail = 0;
    auto prefetch = [&](int t0) {
      const int fr = n - t0 < F ? n - t0 : F, cnt = fr * V;
      const char *p = (const char *)probs + (row0 + (size_t)t0) * (size_t)V * kBytes;
      head = (int)((0u - (unsigned)(uintptr_t)p) & 15u) / kBytes;
      head = head < cnt ? head : cnt;
      nvec = (cnt - head) / kElems;
      tail = cnt - head - nvec * kElems;
      const uint4 *pv = reinterpret_cast<const uint4 *>(p + (size_t)head * kBytes);
#pragma unroll
      for (int u = 0; u < kVecs; ++u) {
        const int iv = tid + kKwThreads * u;
        if (iv < nvec) vq[u] = pv[iv];
      }
      int e = -1;
      if (tid < head) e = tid;
      else if (tid >= 64 && tid - 64 < tail) e = head + nvec * kElems + (tid - 64);
      if (e >= 0) edge = DT == kSkipF32 ? ((const uint32_t *)p)[e] : (uint32_t)((const uint16_t *)p)[e];
      if (tid < fr) m_next = rec[row0 + (size_t)t0 + tid].lp;
    };
    auto put = [&](float *dst, int j, uint32_t raw) {  // element j of the chunk
      const float x = DT == kSkipF32 ? __uint_as_float(raw) : widen_half<DT>(raw);
      dst[j] = rel(to_lp<PROB>(x), s_m[j / V]);
    };
    auto convert = [&](float *dst) {
#pragma unroll
      for (int u = 0; u < kVecs; ++u) {
        const int iv = tid + kKwThreads * u;
        if (iv < nvec) {
          const int j = head + iv * kElems;
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
      if (tid < head) put(dst, tid, edge);
      else if (tid >= 64 && tid - 64 < tail) put(dst, head + nvec * kElems + (tid - 64), edge);
    };
    const int chunk = F * V;
    if (n > 0) {
      prefetch(0);
      if (tid < F) s_m[tid] = m_next;
      __syncthreads();
      convert(s_r);
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
        for (int j = 0; j < F; ++j) me.frame(cur[j * V + col], cur[j * V + blank], t0 + j);
      } else {
        for (int j = 0; j < fr; ++j) me.frame(cur[j * V + col], cur[j * V + blank], t0 + j);
      }
      if (more) {
        if (tid < F) s_m[tid] = m_next;
        __syncthreads();
        convert(s_r + (buf ^ 1) * chunk);
      }
      __syncthreads();  // (the other buffer is complete; this one and s_m are free)
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
        if (t0 + j < n) me.frame(cl[j], __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cb), j)), t0 + j);
    }
  }

  // ---- the result, on the last label's lane; an invalid keyword's on the group's first
  if (me.last || (have && !run && i == 0)) {
    const Hit h = run ? hit_final(me.h) : bad_hit();
    out_sc[out] = h.v;
    out_st[out] = h.s;
    out_en[out] = h.e;
    if (!run && status && b == 0) status[q] = KW_BAD;
  }
  // the traces at and beyond n (an invalid keyword's: everywhere) are 0
  if (have && me.tr_v)
    for (int t = (run ? n : 0) + i; t < T; t += W) {
      me.tr_v[t] = 0.0f;
      me.tr_s[t] = 0;
    }
}

template <int DT, bool PROB, bool STAGED, typename... Args> void launch_one(dim3 grid, size_t lds, hipStream_t s, Args... args) {
  hipLaunchKernelGGL((ctc_keyword_kernel<DT, PROB, STAGED>), grid, dim3(kKwThreads), lds, s, args...);
}
template <int DT, typename... Args> void launch_dt(bool prob, bool staged, dim3 grid, size_t lds, hipStream_t s, Args... args) {
  if (prob && staged) launch_one<DT, true, true>(grid, lds, s, args...);
  else if (prob) launch_one<DT, true, false>(grid, lds, s, args...);
  else if (staged) launch_one<DT, false, true>(grid, lds, s, args...);
  else launch_one<DT, false, false>(grid, lds, s, args...);
}

}  // namespace ctckw

using namespace ctckw;
using ctcalign::align_fail;

extern "C" {

int ctcd_ctc_keywords(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *keywords,
                      const int32_t *keyword_lens, int Q, int L_stride, float *out_scores, int32_t *out_starts, int32_t *out_ends, float *out_end_scores,
                      int32_t *out_end_starts, int32_t *status, void *stream) {
  const std::string f = "ctcd_ctc_keywords: ";
  if (!d) return align_fail(CTCD_EINVAL, "decoder == NULL");
  if (B < 0 || T < 0 || V < 1 || Q < 0 || L_stride < 0) return align_fail(CTCD_EINVAL, (f + "B, T, Q, L_stride >= 0 and V >= 1 required").c_str());
  if (blank_id < 0 || blank_id >= V) return align_fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (log_input < 0 || log_input > 2) return align_fail(CTCD_EINVAL, (f + "log_input must be 0, 1 or 2").c_str());
  if (B == 0 || Q == 0) return CTCD_OK;
  if ((!keywords && L_stride > 0) || !keyword_lens || !out_scores || !out_starts || !out_ends || (T > 0 && !probs) || (!out_end_scores != !out_end_starts))
    return align_fail(CTCD_EINVAL, (f + "null tensor").c_str());
  const bool long_kw = L_stride > kKwMaxLabels && keyword_long_on(d);  // (keyword_long.hip: ctcd_set_long_keywords)
  if (L_stride > kKwMaxLabels && !long_kw) return align_fail(CTCD_EUNSUPPORTED, (f + "keywords of more than 64 labels (L_stride > 64) are not built").c_str());
  if (L_stride > kKwLongMaxLabels) return align_fail(CTCD_EUNSUPPORTED, (f + "keywords of more than 2048 labels (L_stride > 2048) are not built").c_str());
  if (V > (1 << 28)) return align_fail(CTCD_EUNSUPPORTED, (f + "V > 2^28").c_str());
  const int lg = lane_group_log2(L_stride), per_wg = long_kw ? kwl_per_workgroup(kwl_waves(L_stride)) : kw_per_workgroup(lg);
  const long long blocks = ((long long)Q + per_wg - 1) / per_wg;
  if (blocks > 65535) return align_fail(CTCD_EUNSUPPORTED, (f + "too many keywords for one launch").c_str());
  ctcalign::AlignDecoderInfo inf;
  if (const int rc = ctcalign::align_decoder_info(d, &inf)) return rc;
  ctcdev::DeviceGuard guard;
  if (guard.enter(inf.device) != hipSuccess) return align_fail(CTCD_EHIP, (std::string("hipSetDevice: ") + hipGetErrorString(guard.err)).c_str());
  hipStream_t s = (hipStream_t)stream;
  int dtype = inf.in_dtype;
  if (log_input == 2 && T > 0) {  // raw logits: the log-softmax pass into the decoder's float32 rows, then log-probabilities
    const float *rows32 = nullptr;
    if (const int rc = ctcalign::align_lsm_rows(d, probs, seq_lens, B, T, V, stream, &rows32)) return rc;
    probs = rows32;
    dtype = CTCD_DTYPE_F32;
  }
  const bool prob = log_input == 0, staged = kw_staged(V);
  void *rec = nullptr;
  if (T > 0) {
    if (const int rc = ctcgreedy::greedy_scratch(d, ctcgreedy::greedy_scratch_bytes(B, T), &rec)) return rc;
    ctcgreedy::launch_argmax_pass(dtype, prob ? ctcgreedy::kModeProb : ctcgreedy::kModeLog, probs, seq_lens, (long long)B * T, T, V, (FrameRec *)rec, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return align_fail(CTCD_EHIP, (std::string("keyword argmax: ") + hipGetErrorString(e)).c_str());
  }
  const dim3 grid((unsigned)B, (unsigned)blocks);
  const size_t lds = kw_lds_bytes(V);
  const int dt = dtype == CTCD_DTYPE_F16 ? kSkipF16 : (dtype == CTCD_DTYPE_BF16 ? kSkipBF16 : kSkipF32);
  if (long_kw) {
    keyword_note_kernel(d, launch_keyword_long(dt, prob, probs, seq_lens, B, T, V, blank_id, (const FrameRec *)rec, keywords, keyword_lens, Q, L_stride, out_scores,
                                               out_starts, out_ends, out_end_scores, out_end_starts, status, stream));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CTCD_OK : align_fail(CTCD_EHIP, (std::string("long keyword search: ") + hipGetErrorString(e)).c_str());
  }
  auto go = [&](auto tag) {
    launch_dt<decltype(tag)::value>(prob, staged, grid, lds, s, probs, seq_lens, T, V, blank_id, (const FrameRec *)rec, keywords, keyword_lens, Q, L_stride, lg,
                                    out_scores, out_starts, out_ends, out_end_scores, out_end_starts, status);
  };
  if (dt == kSkipF16) go(std::integral_constant<int, kSkipF16>());
  else if (dt == kSkipBF16) go(std::integral_constant<int, kSkipBF16>());
  else go(std::integral_constant<int, kSkipF32>());
  keyword_note_kernel(d, kw_kernel_code(dt, prob, staged, lg));
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CTCD_OK : align_fail(CTCD_EHIP, (std::string("keyword search: ") + hipGetErrorString(e)).c_str());
}

}  // extern "C"
