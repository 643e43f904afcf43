// keyword_long.hip -- keyword search for keywords of 65 .. 2048 labels (include/ctcdecode_amd.h "Keyword search",
// ctcd_set_long_keywords; the shapes are keyword_long.h's, the cell rules keyword.h's).  A translation unit of its own: keyword.hip's
// kernel does not see it, and ctcd_ctc_keywords only dispatches here behind its argmax pass.
//   ctc_keyword_long_kernel<DT, PROB, STAGED>   a workgroup of four waves per item and block of keywords.  A lane holds eight
//       consecutive labels: the label states 2i and the blank states 2i + 1 behind them are 16 (value, start) pairs in its registers.
//       A frame updates them from the lane's last label to its first -- every update reads only cells of the previous frame, so there
//       is no second copy -- with the last label's two pairs of the lane to the left in front (four DPP wave_shr:1 moves a frame).
//     A keyword takes 1, 2 or 4 waves (a runtime argument).  Wave w of a keyword walks one step of Fs frames behind wave w - 1: in
//       iteration `it` of the step loop it walks step it - w.  The last lane of a wave stores its last label's two pairs of every
//       frame into an LDS ring indexed by frame, two steps deep; lane 0 of the next wave reads the entry of frame t while it is at
//       frame t, for frame t + 1.  What is read in an iteration was written in the one before, and what is written lies in the ring's
//       other half: one __syncthreads() an iteration orders them, every wave runs all steps + waves - 1 iterations, and nothing polls.
//     STAGED  (V <= 128): the workgroup stages steps of frames into LDS as r(t, c) -- keyword.hip's 16-byte loads, issued before the
//             iteration's walk and converted behind it -- into a ring of waves + 1 step buffers: a step lives until the keyword's last
//             wave has walked it.  m(t) travels two steps ahead through a two-slot array, so the conversion waits for no barrier of
//             its own.  A lane reads its eight labels' columns and the blank's from LDS.
//     gathered (V > 128): a lane loads its own eight labels' values of the next step's frames into registers a step ahead (lane j of
//             a wave also frame j's blank value and m), converts them when its wave turns to that step and parks them in the wave's
//             private LDS region in keyword order: a frame's eight values come back with two 16-byte reads.  Only the lane that wrote
//             a word reads it, so the region needs no barrier and the skew costs this route nothing.
// Nothing is loaded from HBM on a frame's critical path.  Every store is a plain C++ store; the DPP builtin is the only intrinsic move.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "keyword_long.h"

namespace ctckw {

using ctcskip::kSkipBF16;
using ctcskip::kSkipF16;
using ctcskip::kSkipF32;

namespace kwlong {  // (names of this unit's own: keyword.hip has a Lane and a launch_dt too)

constexpr int E = kKwLongPerLane;

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
__device__ __forceinline__ float lane_value(float x, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j)); }

// a lane's eight labels: their 16 cells, and on the last label's lane the result so far
struct Lane {
  Pair a[E], b[E];  // d[.][2i], d[.][2i + 1] of the labels i = p0 .. p0 + 7
  Pair ca, cb;      // lane 0 of a wave behind another: the left wave's last two cells of the previous frame (the ring's entry)
  Hit h;
  unsigned has2;  // bit e: label e differs from the label in front of it
  bool first;     // the lane of label 0
  bool edge;      // lane 0 of a wave behind another
  bool writer;    // the last lane of a wave in front of another
  int last;       // which of the eight is label len - 1; -1 on every other lane
  int4 *ring_in, *ring_out;
  int ring_mask;
  float *tr_v;  // the keyword's traces at frame 0, or NULL
  int32_t *tr_s;

  __device__ __forceinline__ void frame(const float (&r)[E], float r_blk, int t) {
    Pair la = left_pair(a[E - 1]), lb = left_pair(b[E - 1]);
    if (edge) {
      la = ca;
      lb = cb;
    }
#pragma unroll
    for (int e = E - 1; e >= 0; --e) {  // (a[e - 1], b[e - 1] are still the previous frame's)
      const Pair nb = blank_cell(r_blk, b[e], a[e]);
      a[e] = label_cell(r[e], a[e], e ? b[e - 1] : lb, e ? a[e - 1] : la, (has2 >> e) & 1u, first && e == 0, t);
      b[e] = nb;
    }
    if (writer) ring_out[t & ring_mask] = make_int4(__float_as_int(a[E - 1].v), a[E - 1].s, __float_as_int(b[E - 1].v), b[E - 1].s);
    if (edge) {  // (frame t of the wave in front: written an iteration ago, in the half of the ring that wave has left)
      const int4 x = ring_in[t & ring_mask];
      ca.v = __int_as_float(x.x);
      ca.s = x.y;
      cb.v = __int_as_float(x.z);
      cb.s = x.w;
    }
    if (last >= 0) {
      Pair d = a[0];
#pragma unroll
      for (int e = 1; e < E; ++e)
        if (last == e) d = a[e];
      hit_step(h, d, t);
      if (tr_v) {
        tr_v[t] = d.v;
        tr_s[t] = d.s;
      }
    }
  }
};

template <int DT, bool PROB, bool STAGED>
__global__ void __launch_bounds__(kKwThreads) ctc_keyword_long_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const FrameRec *rec,
                                                                      const int32_t *keywords, const int32_t *keyword_lens, int Q, int L_stride, int waves,
                                                                      float *out_sc, int32_t *out_st, int32_t *out_en, float *out_tr_v, int32_t *out_tr_s,
                                                                      int32_t *status) {
  extern __shared__ __attribute__((aligned(16))) float s_dyn[];  // keyword_long.h kwl_lds_bytes
  __shared__ int4 s_ring[kKwLongWaves - 1][kKwLongRing];         // the boundary behind wave 0, 1, 2 of the workgroup
  __shared__ float s_m[2][kKwLongMaxStep];                       // STAGED: m(t) of the step converted next, and of the one after
  __shared__ int s_bad[kKwLongWaves];                            // per keyword of the workgroup: a lane found it invalid
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = wave & (waves - 1), slot = wave / waves;  // the wave's place in its keyword, the keyword's in the workgroup
  const int q = (int)blockIdx.y * kwl_per_workgroup(waves) + slot;
  const int n = ctcskip::clamped_len(seq_lens, b, T);
  const size_t row0 = (size_t)b * T;
  const int Fs = kwl_step(waves, STAGED), steps = (n + Fs - 1) / Fs, iters = steps ? steps + waves - 1 : 0;
  const int p0 = (w * 64 + lane) * E;  // the lane's first label

  // ---- the keyword: eight labels per lane, validated workgroup-wide before the first frame
  const bool have = q < Q;
  const int len = have ? keyword_lens[q] : 0;
  const bool len_ok = kw_len_ok(len, L_stride);
  const int32_t *kw = keywords + (size_t)(have ? q : 0) * L_stride;
  int lab[E];
  bool bad = have && !len_ok;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    lab[e] = have && p0 + e < L_stride ? kw[p0 + e] : blank;
    if (have && len_ok && p0 + e < len && !ctcalign::label_ok(lab[e], V, blank)) bad = true;
  }
  if (tid < kKwLongWaves) s_bad[tid] = 0;
  __syncthreads();
  if (bad) s_bad[slot] = 1;
  __syncthreads();
  const bool run = have && s_bad[slot] == 0;
  int col[E];  // (always columns of the row)
#pragma unroll
  for (int e = 0; e < E; ++e) col[e] = run && p0 + e < len ? lab[e] : blank;
  // the label in front of the lane's first: the left lane's last, across a wave's edge the keyword's word
  int front = left_i(lab[E - 1]);
  if (lane == 0) front = have && p0 > 0 && p0 - 1 < L_stride ? kw[p0 - 1] : blank;
  const size_t out = (size_t)b * Q + (size_t)(have ? q : 0);
  Lane me;
  me.has2 = 0u;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    me.a[e] = me.b[e] = no_path();
    if (p0 + e > 0 && lab[e] != (e ? lab[e - 1] : front)) me.has2 |= 1u << e;
  }
  me.ca = me.cb = no_path();
  me.h = no_hit();
  me.first = p0 == 0;
  me.edge = lane == 0 && w > 0;
  me.writer = lane == 63 && w < waves - 1;
  me.last = run && len - 1 >= p0 && len - 1 < p0 + E ? len - 1 - p0 : -1;
  me.ring_in = s_ring[wave > 0 ? wave - 1 : 0];
  me.ring_out = s_ring[wave < kKwLongWaves - 1 ? wave : 0];
  me.ring_mask = 2 * Fs - 1;
  me.tr_v = out_tr_v ? out_tr_v + out * T : nullptr;
  me.tr_s = out_tr_v ? out_tr_s + out * T : nullptr;

  if (STAGED) {
    // A step: the frames [t0, t0 + fr) of the item, cnt = fr * V consecutive elements of the input.  Those of them that make up whole
    // aligned 16-byte words are loaded as such (up to four words a thread), the few in front and behind one by one (as in keyword.hip).
    constexpr int kElems = DT == kSkipF32 ? 4 : 8, kBytes = DT == kSkipF32 ? 4 : 2, kVecs = 4;
    uint4 vq[kVecs];
    uint32_t edge = 0u;
    float m_next = 0.0f;
    int head = 0, nvec = 0, tail = 0;
    const int chunk = Fs * V, bufs = kwl_staged_bufs(waves);
    auto load_m = [&](int k) {  // m(t) of step k, a frame a thread
      const int t = k * Fs + tid;
      if (tid < Fs && t < n) m_next = rec[row0 + (size_t)t].lp;
    };
    auto prefetch = [&](int k) {
      const int t0 = k * Fs, fr = n - t0 < Fs ? n - t0 : Fs, cnt = fr * V;
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
    };
    auto convert = [&](int k) {  // what prefetch(k) loaded, into step k's buffer, relative to s_m[k & 1]
      float *dst = s_dyn + (k % bufs) * chunk;
      const float *m = s_m[k & 1];
      auto put = [&](int j, uint32_t raw) {  // element j of the step
        const float x = DT == kSkipF32 ? __uint_as_float(raw) : widen_half<DT>(raw);
        dst[j] = rel(to_lp<PROB>(x), m[j / V]);
      };
#pragma unroll
      for (int u = 0; u < kVecs; ++u) {
        const int iv = tid + kKwThreads * u;
        if (iv < nvec) {
          const int j = head + iv * kElems;
          const uint32_t x[4] = {vq[u].x, vq[u].y, vq[u].z, vq[u].w};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (DT == kSkipF32) {
              put(j + c, x[c]);
            } else {
              put(j + 2 * c, x[c] & 0xffffu);
              put(j + 2 * c + 1, x[c] >> 16);
            }
          }
        }
      }
      if (tid < head) put(tid, edge);
      else if (tid >= 64 && tid - 64 < tail) put(head + nvec * kElems + (tid - 64), edge);
    };
    if (steps > 0) {
      prefetch(0);
      load_m(0);
      if (tid < Fs) s_m[0][tid] = m_next;
      if (steps > 1) load_m(1);
      if (tid < Fs) s_m[1][tid] = m_next;
      __syncthreads();
      convert(0);
      __syncthreads();
    }
    for (int it = 0; it < iters; ++it) {
      const bool more = it + 1 < steps;
      if (more) prefetch(it + 1);  // (in flight while this iteration's steps are walked)
      if (it + 2 < steps) load_m(it + 2);
      const int k = it - w;  // the step this wave walks
      if (run && k >= 0 && k < steps) {
        const float *cur = s_dyn + (k % bufs) * chunk;
        const int t0 = k * Fs, fr = n - t0 < Fs ? n - t0 : Fs;
        for (int j = 0; j < fr; ++j, cur += V) {
          float r[E];
#pragma unroll
          for (int e = 0; e < E; ++e) r[e] = cur[col[e]];
          me.frame(r, cur[blank], t0 + j);
        }
      }
      if (more) convert(it + 1);                   // (its buffer was step it - waves's: walked to the end an iteration ago)
      if (tid < Fs) s_m[it & 1][tid] = m_next;  // m of step it + 2 (the slot's last reader was the conversion of step it)
      __syncthreads();  // (step it + 1 and its m are complete; the ring's entries of this iteration are written)
    }
  } else {
    constexpr int G = kKwLongGatherStep;
    float *mine = s_dyn + (size_t)wave * (G * kKwLongPerWave) + lane * E;  // the lane's eight values of the step's frame 0
    float nl[G][E], nb = 0.0f, nm = 0.0f, rb = 0.0f;
    auto prefetch = [&](int k) {
      const int t0 = k * G;
#pragma unroll
      for (int j = 0; j < G; ++j)
#pragma unroll
        for (int e = 0; e < E; ++e) nl[j][e] = t0 + j < n ? elem_at<DT>(probs, (row0 + (size_t)(t0 + j)) * V + (size_t)col[e]) : 0.0f;
      const int t = t0 + (lane & (G - 1));
      if (t < n) {
        nb = elem_at<DT>(probs, (row0 + (size_t)t) * V + (size_t)blank);
        nm = rec[row0 + (size_t)t].lp;
      }
    };
    auto park = [&]() {  // what prefetch loaded, as r(t, .), into the lane's words of the wave's region
      rb = rel(to_lp<PROB>(nb), nm);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const float m = lane_value(nm, j);
        float4 lo, hi;
        lo.x = rel(to_lp<PROB>(nl[j][0]), m);
        lo.y = rel(to_lp<PROB>(nl[j][1]), m);
        lo.z = rel(to_lp<PROB>(nl[j][2]), m);
        lo.w = rel(to_lp<PROB>(nl[j][3]), m);
        hi.x = rel(to_lp<PROB>(nl[j][4]), m);
        hi.y = rel(to_lp<PROB>(nl[j][5]), m);
        hi.z = rel(to_lp<PROB>(nl[j][6]), m);
        hi.w = rel(to_lp<PROB>(nl[j][7]), m);
        reinterpret_cast<float4 *>(mine + j * kKwLongPerWave)[0] = lo;
        reinterpret_cast<float4 *>(mine + j * kKwLongPerWave)[1] = hi;
      }
    };
    if (run && w == 0 && steps > 0) prefetch(0);
    for (int it = 0; it < iters; ++it) {
      const int k = it - w;  // the step this wave walks; its values were loaded an iteration ago
      const bool walk = run && k >= 0 && k < steps;
      if (walk) park();
      if (run && k + 1 >= 0 && k + 1 < steps) prefetch(k + 1);  // (in flight while this step is walked)
      if (walk) {
#pragma unroll
        for (int j = 0; j < G; ++j)
          if (k * G + j < n) {
            const float4 lo = reinterpret_cast<const float4 *>(mine + j * kKwLongPerWave)[0], hi = reinterpret_cast<const float4 *>(mine + j * kKwLongPerWave)[1];
            const float r[E] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            me.frame(r, lane_value(rb, j), k * G + j);
          }
      }
      __syncthreads();  // (the ring's entries of this iteration are written)
    }
  }

  // ---- the result, on the last label's lane; an invalid keyword's on its first
  if (me.last >= 0 || (have && !run && p0 == 0)) {
    const Hit h = run ? hit_final(me.h) : bad_hit();
    out_sc[out] = h.v;
    out_st[out] = h.s;
    out_en[out] = h.e;
    if (!run && status && b == 0) status[q] = KW_BAD;
  }
  // the traces at and beyond n (an invalid keyword's: everywhere) are 0
  if (have && me.tr_v)
    for (int t = (run ? n : 0) + w * 64 + lane; t < T; t += waves * 64) {
      me.tr_v[t] = 0.0f;
      me.tr_s[t] = 0;
    }
}

template <int DT, bool PROB, bool STAGED, typename... Args> void launch_one(dim3 grid, size_t lds, hipStream_t s, Args... args) {
  hipLaunchKernelGGL((ctc_keyword_long_kernel<DT, PROB, STAGED>), grid, dim3(kKwThreads), lds, s, args...);
}
template <int DT, typename... Args> void launch_dt(bool prob, bool staged, dim3 grid, size_t lds, hipStream_t s, Args... args) {
  if (prob && staged) launch_one<DT, true, true>(grid, lds, s, args...);
  else if (prob) launch_one<DT, true, false>(grid, lds, s, args...);
  else if (staged) launch_one<DT, false, true>(grid, lds, s, args...);
  else launch_one<DT, false, false>(grid, lds, s, args...);
}

}  // namespace kwlong

int launch_keyword_long(int dt, bool prob, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank, const FrameRec *rec, const int32_t *keywords,
                        const int32_t *keyword_lens, int Q, int L_stride, float *out_sc, int32_t *out_st, int32_t *out_en, float *out_tr_v, int32_t *out_tr_s,
                        int32_t *status, void *stream) {
  const int waves = kwl_waves(L_stride), per_wg = kwl_per_workgroup(waves);
  const bool staged = kw_staged(V);
  const dim3 grid((unsigned)B, (unsigned)((Q + per_wg - 1) / per_wg));
  const size_t lds = kwl_lds_bytes(V, waves);
  hipStream_t s = (hipStream_t)stream;
  auto go = [&](auto tag) {
    kwlong::launch_dt<decltype(tag)::value>(prob, staged, grid, lds, s, probs, seq_lens, T, V, blank, rec, keywords, keyword_lens, Q, L_stride, waves, out_sc, out_st, out_en,
                                    out_tr_v, out_tr_s, status);
  };
  if (dt == kSkipF16) go(std::integral_constant<int, kSkipF16>());
  else if (dt == kSkipBF16) go(std::integral_constant<int, kSkipBF16>());
  else go(std::integral_constant<int, kSkipF32>());
  return kwl_kernel_code(dt, prob, staged, waves);
}

}  // namespace ctckw
