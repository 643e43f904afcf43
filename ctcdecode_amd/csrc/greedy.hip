// greedy.hip -- greedy (best-path) CTC decoding of greedy.h on the device, and its C ABI (include/ctcdecode_amd.h "Greedy decode").
// A translation unit of its own, like align.hip: no kernel of ctcdecode_amd.hip or decode_kernels.hip sees it.  Two passes queued
// behind each other on the caller's stream, nothing read on the host in between:
//   the argmax pass: every frame's label c* and lp(t, c*) into the decoder's frame records (8 bytes per frame), in one read of the input
//     greedy_argmax_wave_kernel<DT, MODE>     G = 1 .. 64 lanes per frame (several frames of a short row share a wave), element loads;
//                                             every V, every alignment
//     greedy_argmax_stream_kernel<DT, MODE>   log-probabilities and probabilities: a workgroup per frame, 16-byte loads streamed through
//     greedy_argmax_logits_kernel<F4, DT>     raw logits: a workgroup per frame, the row held in registers between the maximum and the sum
//                                             of exponentials, in the order lsm_device.h fixes; no [B, T, V] copy is written
//   greedy_collapse_kernel                    a workgroup per item: emit and run-end flags, their prefix counts (ballot + popcount per
//                                             wave, wave offsets through LDS, chunks of 1024 frames), the compaction into tokens / starts /
//                                             ends / label_scores, the score chain on one lane, the zero tails
// Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "greedy.h"
#include "lattice_device.h"
#include "lsm_device.h"

namespace ctcgreedy {

using ctcskip::kSkipBF16;
using ctcskip::kSkipF16;
using ctcskip::kSkipF32;

constexpr int kArgmaxThreads = 256;                  // the argmax kernels' workgroup: four waves
constexpr int kCollapseThreads = 1024;               // frames of a collapse chunk = threads of its workgroup (16 waves)
constexpr int kCollapseWaves = kCollapseThreads / 64;
constexpr unsigned kMaxGrid = 1u << 20;              // the argmax kernels stride over the frames beyond it

// exact_math.h's tables, staged into LDS by the workgroups that take logits (Tables::w: [0, 32) exp2f, [32, 48) logf invc, [48, 64) logf logc)
static __device__ const uint64_t kExpTab[32] = CTC_EXP2F_TAB;
static __device__ const double kLogInvc[16] = CTC_LOGF_INVC;
static __device__ const double kLogLogc[16] = CTC_LOGF_LOGC;
__device__ __forceinline__ void stage_tables(uint64_t *s_tbl, int tid) {
  if (tid < 32) s_tbl[tid] = kExpTab[tid];
  else if (tid < 48) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogInvc[tid - 32]);
  else if (tid < 64) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogLogc[tid - 48]);
}

// a half element widened exactly, by the hardware's conversion (the value ctcskip::widen_at gives)
template <int DT> __device__ __forceinline__ float widen_half(uint32_t u16) {
  if (DT == kSkipBF16) return __uint_as_float(u16 << 16);
  return (float)__builtin_bit_cast(_Float16, (uint16_t)u16);
}
template <int DT> __device__ __forceinline__ float elem_at(const void *rows, size_t i) {
  if (DT == kSkipF32) return ((const float *)rows)[i];
  return widen_half<DT>(((const uint16_t *)rows)[i]);
}
// two half elements of one word, in index order
template <int DT> __device__ __forceinline__ void step2(Winner &w, uint32_t word, int c) {
  argmax_step(w, widen_half<DT>(word & 0xffffu), c);
  argmax_step(w, widen_half<DT>(word >> 16), c + 1);
}

// the winner over the lanes lane ^ 1, ^ 2, ... ^ (width / 2): known to all of them
__device__ __forceinline__ Winner group_winner(Winner w, int width) {
  for (int off = 1; off < width; off <<= 1) {
    Winner o;
    o.v = __shfl_xor(w.v, off, 64);
    o.c = __shfl_xor(w.c, off, 64);
    w = argmax_combine(w, o);
  }
  return w;
}
__device__ __forceinline__ void store_rec(FrameRec *rec, long long f, int c, float lp) {
  FrameRec r;
  r.c = c;
  r.lp = lp;
  rec[f] = r;
}
// is frame f one of its item's?  (frames at or beyond the item's length are never read)
__device__ __forceinline__ bool frame_live(long long f, long long frames, const int32_t *seq_lens, int T) {
  if (f >= frames) return false;
  const long long b = f / T;
  return (int)(f - b * T) < ctcskip::clamped_len(seq_lens, (int)b, T);
}

// ---- the argmax pass -----------------------------------------------------------------------------------------------------------------
// G = 1 << lg lanes per frame (greedy.h lanes_per_frame), 64 / G frames per wave; lane g of a frame's group walks the labels g, g + G, ...
// in increasing order.  Raw logits: the sum of exponentials is ctcd_log_softmax's -- lane g adds up its terms in increasing order (for
// V > 64 the 64 chains of the definition; for a shorter row one term, the lanes from V on holding +0) and a butterfly combines the
// group's; what the definition's butterfly adds beyond the group is +0, which changes no sum (every sum holds a term 1).
template <int DT, int MODE>
__global__ void __launch_bounds__(kArgmaxThreads) greedy_argmax_wave_kernel(const void *rows, const int32_t *seq_lens, long long frames, int T, int V, int lg,
                                                                           FrameRec *rec) {
  __shared__ uint64_t s_tbl[64];
  const int tid = (int)threadIdx.x, lane = tid & 63, G = 1 << lg, g = lane & (G - 1);
  if (MODE == kModeLogits) {
    stage_tables(s_tbl, tid);
    __syncthreads();
  }
  const long long per_wave = 64 >> lg, per_wg = per_wave * (kArgmaxThreads / 64);
  for (long long f0 = (long long)blockIdx.x * per_wg; f0 < frames; f0 += (long long)gridDim.x * per_wg) {
    const long long f = f0 + (tid >> 6) * per_wave + (lane >> lg);
    const bool live = frame_live(f, frames, seq_lens, T);  // (the same for the lanes of a group)
    const size_t row0 = (size_t)(live ? f : 0) * (size_t)V;
    Winner w = no_winner();
    if (live)
      for (int j = g; j < V; j += G) argmax_step(w, elem_at<DT>(rows, row0 + (size_t)j), j);
    w = group_winner(w, G);
    float lp;
    if (MODE == kModeLogits) {
      // (no branch around the shuffles: a frame without a finite logit runs the arithmetic on m = 0 and is replaced at the end)
      const float m = lsm_max(w.v), ms = m > neg_inf() ? m : 0.0f;
      float part = 0.0f;
      if (live)
        for (int j = g; j < V; j += G) part += ctcmath::expf_nonpos(elem_at<DT>(rows, row0 + (size_t)j) - ms, s_tbl);
      for (int off = 1; off < G; off <<= 1) part += __shfl_xor(part, off, 64);
      lp = live ? lsm_value(w.v, m, ctcmath::logf_normal(part, s_tbl)) : 0.0f;
    } else {
      lp = w.v;
    }
    if (live && g == 0) store_rec(rec, f, winner_label(w, V), MODE == kModeProb ? winner_lp<kModeProb>(lp) : lp);
  }
}

// the four waves' winners -> the frame's; s_w: the parity's four slots, written by every wave's first lane before the barrier
__device__ __forceinline__ Winner wg_winner(const Winner *s_w) {
  Winner w = s_w[0];
  w = argmax_combine(w, s_w[1]);
  w = argmax_combine(w, s_w[2]);
  return argmax_combine(w, s_w[3]);
}

// Log-probabilities and probabilities of long rows: a workgroup per frame, the row streamed through with 16-byte loads (4 float32 or 8
// half elements; greedy.h vec_rows: V a multiple of that, rows 16-byte aligned), a thread's elements in increasing order.  One barrier per
// frame: the waves' winners alternate between two sets of slots.
template <int DT, int MODE>
__global__ void __launch_bounds__(kArgmaxThreads) greedy_argmax_stream_kernel(const void *rows, const int32_t *seq_lens, long long frames, int T, int V,
                                                                             FrameRec *rec) {
  __shared__ Winner s_w[2][4];
  constexpr int kElems = DT == kSkipF32 ? 4 : 8;
  const int tid = (int)threadIdx.x, nvec = V / kElems;
  int set = 0;
  for (long long f = blockIdx.x; f < frames; f += gridDim.x) {
    if (!frame_live(f, frames, seq_lens, T)) continue;  // (the same for the whole workgroup)
    const uint4 *x = reinterpret_cast<const uint4 *>((const char *)rows + (size_t)f * (size_t)V * ctcskip::elem_bytes(DT));
    Winner w = no_winner();
#pragma unroll 4
    for (int i = tid; i < nvec; i += kArgmaxThreads) {
      const uint4 q = x[i];
      const int c = i * kElems;
      if (DT == kSkipF32) {
        argmax_step(w, __uint_as_float(q.x), c);
        argmax_step(w, __uint_as_float(q.y), c + 1);
        argmax_step(w, __uint_as_float(q.z), c + 2);
        argmax_step(w, __uint_as_float(q.w), c + 3);
      } else {
        step2<DT>(w, q.x, c);
        step2<DT>(w, q.y, c + 2);
        step2<DT>(w, q.z, c + 4);
        step2<DT>(w, q.w, c + 6);
      }
    }
    w = group_winner(w, 64);
    if ((tid & 63) == 0) s_w[set][tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
      w = wg_winner(s_w[set]);
      store_rec(rec, f, winner_label(w, V), winner_lp<MODE>(w.v));
    }
    set ^= 1;
  }
}

// Raw logits of long rows: a workgroup per frame, the row read once with vector loads and held in registers (thread t: the float4s t,
// t + 256, ..., as log_softmax_rows_wg_kernel holds it), so that the maximum and the sum of exponentials are lsm_device.h's, in the
// order ctcd_log_softmax defines.  Requires V % 4 == 0, V <= 1024 * F4, rows aligned to four elements.
template <int F4, int DT>
__global__ void __launch_bounds__(kArgmaxThreads) greedy_argmax_logits_kernel(const void *rows, const int32_t *seq_lens, long long frames, int T, int V,
                                                                             FrameRec *rec) {
  __shared__ uint64_t s_tbl[64];
  __shared__ __attribute__((aligned(16))) ctclsm::LsmLds s;
  __shared__ Winner s_w[4];
  const int tid = (int)threadIdx.x, nv4 = V >> 2;
  stage_tables(s_tbl, tid);
  __syncthreads();
  for (long long f = blockIdx.x; f < frames; f += gridDim.x) {
    if (!frame_live(f, frames, seq_lens, T)) continue;  // (the same for the whole workgroup)
    const char *x = (const char *)rows + (size_t)f * (size_t)V * ctcskip::elem_bytes(DT);
    float4 v[F4];
#pragma unroll
    for (int u = 0; u < F4; ++u) {
      const int i4 = tid + 256 * u;
      v[u] = make_float4(neg_inf(), neg_inf(), neg_inf(), neg_inf());
      if (i4 < nv4) {
        if (DT == kSkipF32) {
          v[u] = reinterpret_cast<const float4 *>(x)[i4];
        } else {
          const uint2 q = reinterpret_cast<const uint2 *>(x)[i4];
          v[u] = make_float4(widen_half<DT>(q.x & 0xffffu), widen_half<DT>(q.x >> 16), widen_half<DT>(q.y & 0xffffu), widen_half<DT>(q.y >> 16));
        }
      }
    }
    Winner w = no_winner();  // (the padding beyond the row is -inf: it never wins)
#pragma unroll
    for (int u = 0; u < F4; ++u) {
      const int c = 4 * (tid + 256 * u);
      argmax_step(w, v[u].x, c);
      argmax_step(w, v[u].y, c + 1);
      argmax_step(w, v[u].z, c + 2);
      argmax_step(w, v[u].w, c + 3);
    }
    const float mine = w.v;  // the thread's maximum, NaN-ignoring as the log-softmax kernels'
    w = group_winner(w, 64);
    if ((tid & 63) == 0) s_w[tid >> 6] = w;
    const float m = ctclsm::wg_row_max(mine, s, tid);  // (contains a barrier: s_w is in place)
    float logsum = 0.0f;
    if (m > neg_inf()) logsum = ctcmath::logf_normal(ctclsm::wg_exp_sum<F4>(v, nv4, m, s, s_tbl, tid), s_tbl);  // (uniform)
    if (tid == 0) {
      w = wg_winner(s_w);
      store_rec(rec, f, winner_label(w, V), lsm_value(w.v, m, logsum));
    }
    __syncthreads();  // (the chunk buffers, wmax and s_w are reused by the next frame)
  }
}

// ---- the collapse pass -----------------------------------------------------------------------------------------------------------------
// One workgroup per item, chunks of kCollapseThreads frames, a frame per thread.  A label's rank = the carry of the chunks before it
// + the flags of the waves before its own (LDS) + those of the lanes before its own (ballot, mbcnt) -- once for the emit flags (tokens,
// starts) and once for the run-end flags (ends, label_scores): the i-th emitting frame and the i-th run end belong to the same label.
// A run's greatest lp: the thread of the run's last frame walks back over the chunk's values in LDS; a run that began in an earlier
// chunk brings its maximum so far along (s_open).  The score chain runs on thread 0, over the chunk's values in LDS.
__device__ __forceinline__ int lanes_before(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
__global__ void __launch_bounds__(kCollapseThreads) greedy_collapse_kernel(const FrameRec *rec, const int32_t *seq_lens, int T, int blank, int32_t *tokens,
                                                                          int32_t *starts, int32_t *ends, float *label_scores, float *scores, int32_t *lens) {
  __shared__ int s_lab[kCollapseThreads];
  __shared__ float s_lp[kCollapseThreads];
  __shared__ int s_cnt[2][kCollapseWaves];  // a chunk's emit | run-end flags per wave
  __shared__ float s_open;                  // the greatest lp so far of the run that is open at the chunk's end
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6;
  const int n = ctcskip::clamped_len(seq_lens, b, T);
  const FrameRec *r = rec + (size_t)b * T;
  int32_t *tok = tokens + (size_t)b * T, *st = starts + (size_t)b * T, *en = ends ? ends + (size_t)b * T : nullptr;
  float *ls = label_scores ? label_scores + (size_t)b * T : nullptr;
  int carry = 0;      // labels emitted by the chunks so far (= the runs that ended in them, + 1 if one is open)
  int carry_end = 0;  // runs ended by the chunks so far
  float score = 0.0f;
  for (int t0 = 0; t0 < n; t0 += kCollapseThreads) {
    const int t = t0 + tid;
    const bool live = t < n;
    FrameRec me;
    me.c = blank;
    me.lp = 0.0f;
    if (live) me = r[t];
    const int before_chunk = t0 > 0 ? r[t0 - 1].c : blank;  // (the label of the frame before the chunk)
    s_lab[tid] = me.c;
    s_lp[tid] = me.lp;
    __syncthreads();
    const int prev = tid > 0 ? s_lab[tid - 1] : before_chunk;
    int next = blank;
    if (t + 1 < n) next = tid + 1 < kCollapseThreads ? s_lab[tid + 1] : r[t + 1].c;
    const bool emit = live && emits(me.c, prev, t == 0, blank), end = live && run_ends(me.c, next, t == n - 1, blank);
    const bool open = live && !end && me.c != blank && tid == kCollapseThreads - 1;  // the run goes on into the next chunk
    float rm = me.lp;
    if (end || open) {
      int k = tid;
      while (k > 0 && s_lab[k - 1] == me.c) {
        --k;
        rm = run_max_back(rm, s_lp[k]);
      }
      if (k == 0 && t0 > 0 && before_chunk == me.c) rm = run_max_back(rm, s_open);
    }
    const unsigned long long m_emit = __ballot(emit), m_end = __ballot(end);
    if ((tid & 63) == 0) {
      s_cnt[0][wave] = __popcll(m_emit);
      s_cnt[1][wave] = __popcll(m_end);
    }
    __syncthreads();
    int below = 0, total = 0, below_end = 0, total_end = 0;
#pragma unroll
    for (int w = 0; w < kCollapseWaves; ++w) {
      const int ce = s_cnt[0][w], cx = s_cnt[1][w];
      below += w < wave ? ce : 0;
      total += ce;
      below_end += w < wave ? cx : 0;
      total_end += cx;
    }
    // (a rank below the number of frames looked at so far: < n <= T)
    if (emit) {
      const int i = carry + below + lanes_before(m_emit);
      tok[i] = me.c;
      st[i] = t;
    }
    if (end) {
      const int i = carry_end + below_end + lanes_before(m_end);
      if (en) en[i] = t;
      if (ls) ls[i] = rm;
    }
    if (open) s_open = rm;
    carry += total;
    carry_end += total_end;
    if (tid == 0) {
      const int cnt = n - t0 < kCollapseThreads ? n - t0 : kCollapseThreads;
#pragma unroll 8
      for (int k = 0; k < cnt; ++k) score = score_step(score, s_lp[k], t0 + k == 0);
    }
    __syncthreads();  // (s_lab, s_lp, s_cnt and s_open are reused by the next chunk)
  }
  if (tid == 0) {
    lens[b] = carry;
    scores[b] = score;
  }
  using ctclattice::zero_words;
  zero_words(tok + carry, T - carry, tid, kCollapseThreads);
  zero_words(st + carry, T - carry, tid, kCollapseThreads);
  if (en) zero_words(en + carry, T - carry, tid, kCollapseThreads);
  if (ls) zero_words(reinterpret_cast<int32_t *>(ls) + carry, T - carry, tid, kCollapseThreads);
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------
template <int DT, int MODE>
void launch_argmax(const void *probs, const int32_t *seq_lens, long long frames, int T, int V, FrameRec *rec, hipStream_t stream) {
  auto grid = [&](long long units) { return dim3((unsigned)(units < (long long)kMaxGrid ? units : (long long)kMaxGrid)); };
  if (!vec_rows((uintptr_t)probs, V, DT, MODE)) {
    const int G = lanes_per_frame(V), lg = __builtin_ctz((unsigned)G);
    const long long per_wg = (long long)(64 / G) * (kArgmaxThreads / 64);
    hipLaunchKernelGGL((greedy_argmax_wave_kernel<DT, MODE>), grid((frames + per_wg - 1) / per_wg), dim3(kArgmaxThreads), 0, stream, probs, seq_lens, frames, T, V,
                       lg, rec);
    return;
  }
  if constexpr (MODE == kModeLogits) {
    auto go = [&](auto f4) {
      hipLaunchKernelGGL((greedy_argmax_logits_kernel<decltype(f4)::value, DT>), grid(frames), dim3(kArgmaxThreads), 0, stream, probs, seq_lens, frames, T, V, rec);
    };
    switch (logits_f4(V)) {
      case 1: go(std::integral_constant<int, 1>()); break;
      case 2: go(std::integral_constant<int, 2>()); break;
      case 4: go(std::integral_constant<int, 4>()); break;
      case 10: go(std::integral_constant<int, 10>()); break;
      default: go(std::integral_constant<int, 16>());
    }
  } else {
    hipLaunchKernelGGL((greedy_argmax_stream_kernel<DT, MODE>), grid(frames), dim3(kArgmaxThreads), 0, stream, probs, seq_lens, frames, T, V, rec);
  }
}
template <int DT>
void launch_argmax_mode(int mode, const void *probs, const int32_t *seq_lens, long long frames, int T, int V, FrameRec *rec, hipStream_t stream) {
  if (mode == kModeProb) launch_argmax<DT, kModeProb>(probs, seq_lens, frames, T, V, rec, stream);
  else if (mode == kModeLog) launch_argmax<DT, kModeLog>(probs, seq_lens, frames, T, V, rec, stream);
  else launch_argmax<DT, kModeLogits>(probs, seq_lens, frames, T, V, rec, stream);
}
// the argmax pass over [frames / T, T, V] rows of the element type in_dtype (CTCD_DTYPE_*): greedy_stream.hip launches it too
void launch_argmax_pass(int in_dtype, int mode, const void *probs, const int32_t *seq_lens, long long frames, int T, int V, FrameRec *rec, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (in_dtype == CTCD_DTYPE_F16) launch_argmax_mode<kSkipF16>(mode, probs, seq_lens, frames, T, V, rec, s);
  else if (in_dtype == CTCD_DTYPE_BF16) launch_argmax_mode<kSkipBF16>(mode, probs, seq_lens, frames, T, V, rec, s);
  else launch_argmax_mode<kSkipF32>(mode, probs, seq_lens, frames, T, V, rec, s);
}

}  // namespace ctcgreedy

using namespace ctcgreedy;
using ctcalign::align_fail;

extern "C" {

int ctcd_greedy_decode(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, int32_t *out_tokens,
                       int32_t *out_starts, int32_t *out_ends, float *out_label_scores, float *out_scores, int32_t *out_lens, void *stream) {
  const std::string f = "ctcd_greedy_decode: ";
  if (!d) return align_fail(CTCD_EINVAL, "decoder == NULL");
  if (B < 0 || T < 0 || V < 1) return align_fail(CTCD_EINVAL, (f + "B, T >= 0 and V >= 1 required").c_str());
  if (blank_id < 0 || blank_id >= V) return align_fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (log_input < 0 || log_input > 2) return align_fail(CTCD_EINVAL, (f + "log_input must be 0, 1 or 2").c_str());
  if (B == 0) return CTCD_OK;
  if (!out_scores || !out_lens || (T > 0 && (!probs || !out_tokens || !out_starts))) return align_fail(CTCD_EINVAL, (f + "null tensor").c_str());
  if (V > (1 << 28)) return align_fail(CTCD_EUNSUPPORTED, (f + "V > 2^28").c_str());
  ctcalign::AlignDecoderInfo inf;
  if (const int rc = ctcalign::align_decoder_info(d, &inf)) return rc;
  ctcdev::DeviceGuard guard;
  if (guard.enter(inf.device) != hipSuccess) return align_fail(CTCD_EHIP, (std::string("hipSetDevice: ") + hipGetErrorString(guard.err)).c_str());
  hipStream_t s = (hipStream_t)stream;
  void *rec = nullptr;
  if (T > 0) {
    if (const int rc = greedy_scratch(d, greedy_scratch_bytes(B, T), &rec)) return rc;
    launch_argmax_pass(inf.in_dtype, log_input, probs, seq_lens, (long long)B * T, T, V, (FrameRec *)rec, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return align_fail(CTCD_EHIP, (std::string("greedy argmax: ") + hipGetErrorString(e)).c_str());
  }
  hipLaunchKernelGGL(greedy_collapse_kernel, dim3((unsigned)B), dim3(kCollapseThreads), 0, s, (const FrameRec *)rec, seq_lens, T, blank_id, out_tokens, out_starts,
                     out_ends, out_label_scores, out_scores, out_lens);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CTCD_OK : align_fail(CTCD_EHIP, (std::string("greedy collapse: ") + hipGetErrorString(e)).c_str());
}

}  // extern "C"
