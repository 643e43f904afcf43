// prepass.hip -- the pre-pass kernels: what runs on the caller's rows in front of the decode kernel (prepass.h).  A translation unit
// of its own, like the features' units: an edit of the library's host file (ctcdecode_amd.hip) compiles none of these hundred
// instantiations again, and an edit here touches no host code.  The kernels and their device helpers stay in the unnamed namespace;
// the host reaches them through the kPrepass table at the end of this file, which holds their addresses, and through launch_order.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/ctcdecode_amd.h"
#include "decode_kernel.h"
#include "exact_math_f64.h"
#include "lsm_device.h"
#include "prepass.h"

namespace {

using namespace ctcbeam;
using namespace ctcdk;  // (the wave-level scans of decode_kernel.h: wave_sum, wave_min, CTC_DPP)
using namespace ctcprepass;

// The data of the bit-exact binary64 log / exp (exact_math_f64.h): the vocabulary pruning and the probability -> log
// conversion evaluate exactly what the reference's C library evaluates (decoder_utils.cpp:16,29,42), on the device.
#define g_t64 (ctcmath::tables64())

// Element type of the caller's rows (ctcd_set_input_dtype): float32, or IEEE binary16 / bfloat16.  Every pre-pass kernel is a template
// on DT and reads its rows through in_at / in_load4 alone, which widen a half element to float as they read it (exact: the kernels
// compute on the very float values they would read from x.float()); four half elements come with one 8-byte load where float32 rows
// take a float4, so the thread-to-label mapping, and with it the summation order that defines the log-softmax, is the same for every
// DT.  Nothing behind the pre-passes (candidate lists, the decode kernels) sees the type.
enum InDtype { kInF32 = CTCD_DTYPE_F32, kInF16 = CTCD_DTYPE_F16, kInBF16 = CTCD_DTYPE_BF16 };
template <int DT> struct InElem { using T = uint16_t; };  // (DT = kInF16 / kInBF16)
template <> struct InElem<kInF32> { using T = float; };
template <int DT> __device__ __forceinline__ float widen_in(uint16_t u) {
  if (DT == kInBF16) return __uint_as_float((uint32_t)u << 16);
  return (float)__builtin_bit_cast(_Float16, u);
}
template <int DT, typename I> __device__ __forceinline__ float in_at(const typename InElem<DT>::T *row, I i) {
  if constexpr (DT == kInF32) return row[i];
  else return widen_in<DT>(row[i]);
}
// elements 4 * i4 .. 4 * i4 + 3 of a row (16-byte aligned for float32, 8-byte for half rows).  (float32: a reference to the element,
// not a copy returned by value -- the copy is loaded as four floats instead of two float2s, and the kernels' machine code changes)
template <int DT> __device__ __forceinline__ decltype(auto) in_load4(const typename InElem<DT>::T *row, int i4) {
  if constexpr (DT == kInF32) {
    return reinterpret_cast<const float4 *>(row)[i4];
  } else {
    const uint2 w = reinterpret_cast<const uint2 *>(row)[i4];
    return make_float4(widen_in<DT>((uint16_t)(w.x & 0xffffu)), widen_in<DT>((uint16_t)(w.x >> 16)), widen_in<DT>((uint16_t)(w.y & 0xffffu)),
                       widen_in<DT>((uint16_t)(w.y >> 16)));
  }
}
template <int DT> __device__ __forceinline__ const typename InElem<DT>::T *in_rows(const float *p) {  // (the kernels' row pointers are typed float)
  return reinterpret_cast<const typename InElem<DT>::T *>(p);
}

// prob -> log-prob exactly as decoder_utils.cpp:42 : float(log(double(p) + FLT_MIN)), every element, bit for bit.
// (Rounds 1-3 used the device library's log() and sent the elements whose float rounding it could not guarantee through
//  the host's libm; the restated routine needs no second opinion.)
template <int DT>
__global__ void prob_to_log_kernel(const float *in_, float *out, size_t n, const int32_t *seq_lens, int T, int V) {
  const typename InElem<DT>::T *in = in_rows<DT>(in_);
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t tv = (size_t)T * V;
  for (; i < n; i += stride) {
    if (seq_lens) {  // frames beyond the utterance's length are never read by the reference (binding.cpp:64-65)
      const size_t b = i / tv;
      const int t = (int)((i - b * tv) / (size_t)V);
      if (t >= seq_lens[b]) continue;
    }
    out[i] = (float)ctcmath::log_f64((double)in_at<DT>(in, i) + (double)FLT_MIN, g_t64);
  }
}

// Half rows widened to float32 into the decoder's workspace, where a decode kernel reads the caller's rows itself (log-probability
// rows without pruning; the LM tier's blank values).  Frames past an utterance's end are skipped as above.
template <int DT>
__global__ void widen_rows_kernel(const float *in_, float *out, size_t n, const int32_t *seq_lens, int T, int V) {
  const typename InElem<DT>::T *in = in_rows<DT>(in_);
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t tv = (size_t)T * V;
  for (; i < n; i += stride) {
    if (seq_lens) {
      const size_t b = i / tv;
      const int t = (int)((i - b * tv) / (size_t)V);
      if (t >= seq_lens[b]) continue;
    }
    out[i] = in_at<DT>(in, i);
  }
}

// Raw-logit input (log_input == 2, an extension: the reference's callers run log_softmax themselves): one wave per frame,
//   y_j = (x_j - m) - logf(s),  m = max_j x_j (a zero maximum taken as +0),  s = sum_j expf(x_j - m) in float32,
// where lane l first adds up the terms j = l, l + 64, ... in increasing j and the 64 partial sums are then combined by a
// butterfly (lane ^ 1, ^ 2, ... ^ 32); expf / logf are the bit-exact restatements of exact_math.h (expf below -88 is 0).
// The order of the additions is part of the definition: tests/native/core_host.cpp computes the same thing with the C
// library, bit for bit.  A frame without a finite logit yields -inf everywhere.
template <int DT>
__global__ void __launch_bounds__(256) log_softmax_rows_kernel(const float *in_, float *out, long long rows, const int32_t *seq_lens, int T, int V,
                                                               const uint64_t *tables) {
  const typename InElem<DT>::T *in = in_rows<DT>(in_);
  __shared__ uint64_t tbl[64];
  if (threadIdx.x < 64) tbl[threadIdx.x] = tables[threadIdx.x];
  __syncthreads();
  const int lane = (int)threadIdx.x & 63;
  const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
  for (long long r = wave0; r < rows; r += nwaves) {
    if (seq_lens) {  // frames beyond the utterance's length are never read (binding.cpp:64-65)
      const long long b = r / T;
      if ((int)(r - b * T) >= seq_lens[b]) continue;
    }
    const typename InElem<DT>::T *x = in + (size_t)r * V;
    float *y = out + (size_t)r * V;
    float m = -INFINITY;
    for (int j = lane; j < V; j += 64) { const float v = in_at<DT>(x, j); m = v > m ? v : m; }
    for (int off = 1; off < 64; off <<= 1) { const float o = __shfl_xor(m, off, 64); m = o > m ? o : m; }
    m += 0.0f;  // (a zero maximum is +0)
    if (!(m > -INFINITY)) {
      for (int j = lane; j < V; j += 64) y[j] = -INFINITY;
      continue;
    }
    float part = 0.0f;
    for (int j = lane; j < V; j += 64) part += ctcmath::expf_nonpos(in_at<DT>(x, j) - m, tbl);
    for (int off = 1; off < 64; off <<= 1) part += __shfl_xor(part, off, 64);
    const float ls = ctcmath::logf_normal(part, tbl);
    for (int j = lane; j < V; j += 64) y[j] = (in_at<DT>(x, j) - m) - ls;
  }
}

// The same normalisation for long rows, shaped for HBM bandwidth: one workgroup of four waves per frame, the row read ONCE
// with 128-bit loads and held in registers (thread t: the float4s t, t + 256, ...), written once.  The sum keeps the order
// the definition fixes; lsm_device.h has the helpers that see to it (wg_row_max, wg_exp_sum, LsmLds), shared with the greedy
// decode's logit kernel (greedy.hip).  Requires V % 4 == 0 and V <= 1024 * F4.
using ctclsm::LsmLds;
using ctclsm::wg_exp_sum;
using ctclsm::wg_row_max;
template <int F4, int DT>
__global__ void __launch_bounds__(256, F4 <= 10 ? 5 : 4) log_softmax_rows_wg_kernel(const float *in_, float *out, long long rows, const int32_t *seq_lens, int T,
                                                                                     int V, const uint64_t *tables) {
  __shared__ uint64_t tbl[64];
  __shared__ __attribute__((aligned(16))) LsmLds s;
  const typename InElem<DT>::T *in = in_rows<DT>(in_);
  const int tid = (int)threadIdx.x, nv4 = V >> 2;
  if (tid < 64) tbl[tid] = tables[tid];
  __syncthreads();
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    if (seq_lens) {  // frames beyond the utterance's length are never read (binding.cpp:64-65)
      const long long b = r / T;
      if ((int)(r - b * T) >= seq_lens[b]) continue;
    }
    const typename InElem<DT>::T *x4 = in + (size_t)r * V;
    float4 *y4 = reinterpret_cast<float4 *>(out + (size_t)r * V);
    int tq = tid;  // (opaque per frame: the chunks' predicates and offsets are recomputed, not kept across the frame loop)
    asm volatile("" : "+v"(tq));
    float4 v[F4];
#pragma unroll
    for (int u = 0; u < F4; ++u) {
      const int i4 = tq + 256 * u;
      v[u] = i4 < nv4 ? in_load4<DT>(x4, i4) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    }
    float mine = -INFINITY;
#pragma unroll
    for (int u = 0; u < F4; ++u) {
      mine = v[u].x > mine ? v[u].x : mine; mine = v[u].y > mine ? v[u].y : mine;
      mine = v[u].z > mine ? v[u].z : mine; mine = v[u].w > mine ? v[u].w : mine;
    }
    const float m = wg_row_max(mine, s, tid);
    if (!(m > -INFINITY)) {
#pragma unroll
      for (int u = 0; u < F4; ++u)
        if (tq + 256 * u < nv4) y4[tq + 256 * u] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    } else {
      const float ls = ctcmath::logf_normal(wg_exp_sum<F4>(v, nv4, m, s, tbl, tq), tbl);
#pragma unroll
      for (int u = 0; u < F4; ++u)
        if (tq + 256 * u < nv4) y4[tq + 256 * u] = make_float4((v[u].x - m) - ls, (v[u].y - m) - ls, (v[u].z - m) - ls, (v[u].w - m) - ls);
    }
    __syncthreads();  // (the chunk buffers and wmax are reused by the next frame)
  }
}

// ------------------------------------------------------------------------------------------------ vocabulary prune
// get_pruned_log_probs (decoder_utils.cpp:10-45) for every frame, one wave per frame, no barriers: the top
// min(cutoff_top_n, V) values in descending order (and, with cutoff_prob < 1, the reference's cumulative cut).
// The order std::sort gives EQUAL values is toolchain behaviour the reference inherits, and its cumulative cut is a
// sequential chain of binary64 log / exp: whenever a frame's result could depend on either (equal values at or above the
// cut, a cumulative sum within rounding distance of cutoff_prob) the frame is flagged and settled by prune_resolve_kernel
// -- on the device: a replay of libstdc++'s std::sort and the chain with the bit-exact log / exp of exact_math_f64.h.
// Everything else is decided here, exactly (the kept probabilities' logs with the same bit-exact log).
// NaN: the reference's comparator is not a strict weak order on rows that hold one (its std::sort call is undefined
// behaviour there); here a NaN ranks below every number, -inf included, and is otherwise carried through.
// (kPruneCand, the capacity of the pre-filter candidate list per frame, and PruneArgs: prepass.h)

// log_input == 2: the value the prune ranks is the frame's log-softmax (x - m) - ls, never stored as a row; m = -inf (no finite
// logit): -inf everywhere, as log_softmax_rows_kernel defines it
__device__ __forceinline__ float prune_row_value(const PruneArgs &a, float x, float m, float ls) {
  if (a.log_input != 2) return x;
  return m > -INFINITY ? (x - m) - ls : -INFINITY;
}

__device__ __forceinline__ uint32_t prune_key(float v) {  // order of the doubles the reference compares; -0 == +0
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 1u;  // NaN: below every number (key 0 = no element)
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Inclusive prefix sum of a double over the 64 lanes of a wave with DPP moves on the two halves of the value (a
// ds_bpermute-based shuffle costs an LDS round trip per step; this runs while the other waves of the workgroup wait).
__device__ __forceinline__ double f64_dpp(double v, const int ctrl_sel) {
  union { double d; int i[2]; } in, out;
  in.d = v;
  switch (ctrl_sel) {  // (the DPP control word is an immediate)
    case 0: out.i[0] = CTC_DPP(0, in.i[0], 0x111, 0xf); out.i[1] = CTC_DPP(0, in.i[1], 0x111, 0xf); break;  // row_shr:1
    case 1: out.i[0] = CTC_DPP(0, in.i[0], 0x112, 0xf); out.i[1] = CTC_DPP(0, in.i[1], 0x112, 0xf); break;  // row_shr:2
    case 2: out.i[0] = CTC_DPP(0, in.i[0], 0x114, 0xf); out.i[1] = CTC_DPP(0, in.i[1], 0x114, 0xf); break;  // row_shr:4
    case 3: out.i[0] = CTC_DPP(0, in.i[0], 0x118, 0xf); out.i[1] = CTC_DPP(0, in.i[1], 0x118, 0xf); break;  // row_shr:8
    case 4: out.i[0] = CTC_DPP(0, in.i[0], 0x142, 0xa); out.i[1] = CTC_DPP(0, in.i[1], 0x142, 0xa); break;  // row_bcast:15 -> rows 1, 3
    default: out.i[0] = CTC_DPP(0, in.i[0], 0x143, 0xc); out.i[1] = CTC_DPP(0, in.i[1], 0x143, 0xc); break; // row_bcast:31 -> rows 2, 3
  }
  return out.d;  // (lanes without a source receive +0.0: the identity)
}
__device__ __forceinline__ double wave_scan_f64_sum(double v) {
  v += f64_dpp(v, 0); v += f64_dpp(v, 1); v += f64_dpp(v, 2); v += f64_dpp(v, 3); v += f64_dpp(v, 4); v += f64_dpp(v, 5);
  return v;
}
__device__ __forceinline__ double f64_from_lane(double v, int lane_idx) {
  union { double d; int i[2]; } in, out;
  in.d = v;
  out.i[0] = __builtin_amdgcn_readlane(in.i[0], lane_idx); out.i[1] = __builtin_amdgcn_readlane(in.i[1], lane_idx);
  return out.d;
}

__device__ __forceinline__ double log_add_f64(double a, double b) {  // decoder_utils.h:47-54 with T = double
  const double neg = -1.7976931348623157e308;
  if (a <= neg) return b;
  if (b <= neg) return a;
  const double m = a > b ? a : b;
  return log(exp(a - m) + exp(b - m)) + m;
}

// Half rows (DT != kInF32): rows of fp16 / bf16 values tie in almost every frame, and a tie flags a frame here only if it can change
// the result.  The kept length after the cumulative cut (decoder_utils.cpp:26-31) does not depend on the order std::sort gives equal
// values: cum_prob adds the sorted values, and equal values give the same partial sums in any order.  So the cut is computed first
// and a group of equal values flags the frame only when one of its members lies inside the kept length -- it then either straddles
// that length or has two members inside it; with a single member inside, the group reaches beyond.  Put the other way: with first_tie
// the first sorted position that belongs to a group of equal values, the frame is settled here iff the cut stops at or before
// first_tie, and positions [0, first_tie) hold distinct values whose order and conversion are fixed.  The cut can only stop early for
// cutoff_prob < ln 2 (cum_prob starts at 0.0 = log 1: PruneArgs::cut_exp); at the default 0.99 the kept length is cutoff_top_n and
// the rule flags exactly what the float32 rule flags.  (float32 rows keep the rule that flags every tie inside cutoff_top_n.)

// R > 0: the frame's keys are held in registers (64*R >= V); R == 0: re-read from memory on every pass.
template <int R, int DT>
__global__ void __launch_bounds__(256) prune_rows_kernel(PruneArgs a) {
  const typename InElem<DT>::T *in = in_rows<DT>(a.in);
  extern __shared__ __attribute__((aligned(16))) char psm[];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, wpb = (int)blockDim.x >> 6;
  const int n = a.top_n < a.V ? a.top_n : a.V;
  // per wave: kept keys, labels, labels in final order (stride each); pre-filter candidates (keys, labels)
  uint32_t *lkey = (uint32_t *)psm + (size_t)wave * (3 * a.stride + 2 * kPruneCand);
  int *lidx = (int *)lkey + a.stride;
  int *sidx = lidx + a.stride;
  uint32_t *ckey = (uint32_t *)(sidx + a.stride);
  int *cidx = (int *)ckey + kPruneCand;
  for (long long r = (long long)blockIdx.x * wpb + wave; r < a.rows; r += (long long)gridDim.x * wpb) {
    if (a.seq_lens) {  // frames beyond the utterance's length are never read (binding.cpp:64-65)
      const long long b = r / a.T;
      int len = a.seq_lens[b];
      len = len < 0 ? 0 : len;
      if ((int)(r - b * a.T) >= len) continue;
    }
    const typename InElem<DT>::T *x = in + (size_t)r * a.V;
    bool flag = false;
    // (half rows: equal values inside cutoff_top_n -- flag the frame only if the cut reaches them.  Where the keep tests and the
    //  final flag read it, a constant condition on DT leaves it out of the float32 code: a `tie` the optimiser folds away later
    //  would still change the float32 kernels' machine code)
    bool tie = false;
    int first_tie = a.V;  // ... the first sorted position of such a group
    uint32_t keys[R > 0 ? R : 1];
    if (R > 0) {
#pragma unroll
      for (int u = 0; u < R; ++u) keys[u] = lane + 64 * u < a.V ? prune_key(in_at<DT>(x, lane + 64 * u)) : 0u;  // 0 < every real key
    }
    uint32_t tau = 0;
    int g = 0, e = 0, base = 0;
    bool done = false;
    if (R > 0 && n <= 64) {
      // Pre-filter: tau is at least the n-th largest of the 64 per-lane maxima (those are n elements >= it), so only
      // keys >= that bound (a few dozen of V) can be among the top n.  They are listed in LDS and ranked exactly.
      uint32_t lmax = 0;
#pragma unroll
      for (int u = 0; u < R; ++u) lmax = keys[u] > lmax ? keys[u] : lmax;
      uint32_t bound = 0;
      for (int bit = 31; bit >= 0; --bit) {
        const uint32_t trial = bound | (1u << bit);
        if (__popcll(__ballot(lmax >= trial)) >= n) bound = trial;
      }
      int ns = 0;
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const bool in = keys[u] >= bound && keys[u] != 0u;
        const unsigned long long m = __ballot(in);
        if (m) {
          const int p = ns + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          if (in && p < kPruneCand) { ckey[p] = keys[u]; cidx[p] = lane + 64 * u; }
          ns += __popcll(m);
        }
      }
      if (ns <= kPruneCand) {
        // exact n-th largest among the ns candidates (every lane ranks its own candidates against all of them)
        uint32_t found = 0;
        for (int q = lane; q < ns; q += 64) {
          const uint32_t mine = ckey[q];
          int gg = 0, ee = 0;
          for (int o = 0; o < ns; ++o) {
            const uint32_t k = ckey[o];
            gg += k > mine;
            ee += k == mine;
          }
          if (gg < n && n <= gg + ee) found = mine;
        }
        const unsigned long long mf = __ballot(found != 0u);
        tau = (uint32_t)__builtin_amdgcn_readlane((int)found, __ffsll((long long)mf) - 1);
        for (int q = lane; q < ns; q += 64) { g += ckey[q] > tau; e += ckey[q] == tau; }
        g = wave_sum(g);
        e = wave_sum(e);
        if (e > n - g) {  // equal values straddle the cut: std::sort decides which of them are kept
          if constexpr (DT == kInF32) flag = true;
          else { tie = true; first_tie = g; }
        }
        for (int q0 = 0; q0 < ns; q0 += 64) {
          const int q = q0 + lane;
          const uint32_t k = q < ns ? ckey[q] : 0u;
          const bool keep = q < ns && (k > tau || (k == tau && (DT == kInF32 ? !flag : !(flag || tie))));
          const unsigned long long m = __ballot(keep);
          if (keep) {
            const int p = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            lkey[p] = k;
            lidx[p] = cidx[q];
          }
          base += __popcll(m);
        }
        done = true;
      }
    }
    if (!done) {
      // n-th largest key, bit by bit, over all V values
      for (int bit = 31; bit >= 0; --bit) {
        const uint32_t trial = tau | (1u << bit);
        int c = 0;
        if (R > 0) {
#pragma unroll
          for (int u = 0; u < R; ++u) c += keys[u] >= trial;
        } else {
          for (int i = lane; i < a.V; i += 64) c += prune_key(in_at<DT>(x, i)) >= trial;
        }
        if (wave_sum(c) >= n) tau = trial;
      }
      if (R > 0) {
#pragma unroll
        for (int u = 0; u < R; ++u) { g += keys[u] > tau; e += keys[u] == tau; }
      } else {
        for (int i = lane; i < a.V; i += 64) {
          const uint32_t k = prune_key(in_at<DT>(x, i));
          g += k > tau;
          e += k == tau;
        }
      }
      g = wave_sum(g);
      e = wave_sum(e);
      if (e > n - g) {  // equal values straddle the cut: std::sort decides which of them are kept
        if constexpr (DT == kInF32) flag = true;
        else { tie = true; first_tie = g; }
      }
      // gather the kept values
      auto take = [&](int i, uint32_t k, bool valid) {
        const bool keep = valid && (k > tau || (k == tau && (DT == kInF32 ? !flag : !(flag || tie))));
        const unsigned long long m = __ballot(keep);
        if (keep) {
          const int p = base + __popcll(m & ((1ull << lane) - 1ull));
          lkey[p] = k;
          lidx[p] = i;
        }
        base += __popcll(m);
      };
      if (R > 0) {
#pragma unroll
        for (int u = 0; u < R; ++u) take(lane + 64 * u, keys[u], lane + 64 * u < a.V);
      } else {
        for (int i0 = 0; i0 < a.V; i0 += 64) {
          const int i = i0 + lane;
          take(i, i < a.V ? prune_key(in_at<DT>(x, i)) : 0u, i < a.V);
        }
      }
    }
    const int kept = base;  // == n unless flagged
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS writes are visible to its other lanes
    // rank (descending); equal kept values -> their order is std::sort's business
    int *och = a.ch + (size_t)r * a.stride;
    float *olp = a.lp + (size_t)r * a.stride;
    for (int q = lane; q < kept; q += 64) {
      const uint32_t mine = lkey[q];
      int rank = 0, dup = 0;
      for (int o = 0; o < kept; ++o) {
        const uint32_t k = lkey[o];
        rank += k > mine;
        dup += k == mine;
      }
      if (dup > 1) {
        if constexpr (DT == kInF32) flag = true;
        else { tie = true; first_tie = rank < first_tie ? rank : first_tie; }
      }
      const int idx = lidx[q];
      float v = in_at<DT>(x, idx);
      if (!a.log_input) {  // decoder_utils.cpp:42
        v = (float)ctcmath::log_f64((double)v + (double)FLT_MIN, g_t64);
      }
      if (dup <= 1) { och[rank] = idx; olp[rank] = v; sidx[rank] = idx; }
    }
    flag = __ballot(flag) != 0ull;
    int len = kept;
    int cut_n = kept;  // entries the cut may walk: half rows with a tie stop before its first member
    if constexpr (DT != kInF32) {
      tie = __ballot(tie) != 0ull;
      first_tie = wave_min(first_tie);
      if (tie && !flag) {
        if (a.cutoff_prob < 1.0) cut_n = first_tie;
        else flag = true;  // (no cut: the kept length is cutoff_top_n, and the tie lies inside it)
      }
    }
    bool cut_hit = false;
    if (a.cutoff_prob < 1.0 && !flag) {
      // decoder_utils.cpp:25-32: cum = log_sum_exp(cum, log p_i) starting from cum = 0.0 (sic), i.e. after i+1 terms
      // cum = log(1 + p_0 + ... + p_i); keep going until cum >= cutoff_prob or cutoff_top_n entries.  Evaluated here
      // as a wave-parallel prefix sum (differs from the reference's sequential double chain by ~1e-14 relative); a
      // frame where any partial sum comes within 1e-9 of the threshold is left to prune_resolve_kernel's exact chain.
      int stop = cut_n;  // number of entries kept
      double carry = 0.0;
      for (int i0 = 0; i0 < cut_n && stop == cut_n; i0 += 64) {
        const int i = i0 + lane;
        double p = 0.0;
        if (i < cut_n) {
          const double v = (double)in_at<DT>(x, sidx[i]);
          p = a.log_input ? exp(v) : v;
        }
        double incl = p;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const double o = __shfl_up(incl, off, 64);
          if (lane >= off) incl += o;
        }
        const double cum = log(1.0 + carry + incl);
        const bool near = i < cut_n && (fabs(cum - a.cutoff_prob) <= 1e-9 * (1.0 + fabs(cum)) || !(cum == cum));
        const bool hit = i < cut_n && (cum >= a.cutoff_prob || i + 1 >= a.top_n);
        const unsigned long long mh = __ballot(hit), mn = __ballot(near);
        const int firsthit = mh ? __ffsll((long long)mh) - 1 : 64;
        if (mn && (__ffsll((long long)mn) - 1) <= firsthit) flag = true;  // ambiguous before (or at) the stopping point
        if (mh) { stop = i0 + firsthit + 1; cut_hit = true; }
        carry += f64_from_lane(incl, 63);
      }
      len = stop;
      flag = __ballot(flag) != 0ull;
    }
    if (DT != kInF32 && tie && !cut_hit) flag = true;  // the kept length reaches the first group of equal values
    if (lane == 0) {
      a.cnt[r] = len;
      if (flag) {
        const unsigned k = atomicAdd(a.n_flag, 1u);
        if (k < a.flag_cap) a.flag_rows[k] = (unsigned)r;
      }
    }
  }
}

// The same pass for large vocabularies, shaped for HBM bandwidth (the one genuinely HBM-bound kernel of this library:
// V * 4 bytes read per frame, 8 * top_n + 4 written).  One workgroup of four waves per frame, two sweeps over the row
// with 128-bit loads: the first keeps only every thread's maximum (a lower bound of the n-th largest value follows from
// the lanes' maxima: in each wave the ceil(n/4)-th largest of its 64 lane maxima, to 20 bits; the smallest of the four
// wave bounds has at least n values above it), the second -- served by L2, the row was just read -- lists the few
// dozen values at or above the bound in LDS, where wave 0 ranks them exactly.  Ties, the cumulative cut and the log
// conversion are decided as in prune_rows_kernel above.  Few registers per thread (nothing of the row is kept), so
// eight workgroups share a CU and hide each other's latencies.
// Requires V % 4 == 0 (rows aligned to four elements), V <= 1024 * F4, cutoff_top_n <= 64.
// decoder_utils.cpp:25-32 for one frame, by one wave: the kept candidates (sidx[0, kept): their labels, best first) are cut
// where the running sum of their probabilities reaches cutoff_prob (the reference accumulates log(1 + sum): its running
// value starts at 0.0 in log space).  This is the fast form -- a wave-parallel prefix sum and the device library's
// exp()/log(), not the reference's sequential chain: whenever the comparison with cutoff_prob could go either way before (or
// at) the stopping point, `flag` is raised and prune_resolve_kernel walks the chain exactly (prune_exact_cut).
__device__ __forceinline__ int prune_cumulative_cut(const PruneArgs &a, const float *x, const int *sidx, int kept, int lane, bool &flag, const uint64_t *tbl) {
  // cum = log(1 + sum) >= cutoff_prob  <=>  1 + sum >= exp(cutoff_prob) (a.cut_exp, from the host's libm): no logarithm here, and
  // the probabilities of log-probability rows from expf's own evaluation kept in binary64 (exact_math.h expf_core_f64, ~2e-10):
  // sums within 1e-8 of the threshold -- fifty times that error -- are not decided here.  (The device library's exp() / log(),
  // used until round 5, cost the kernels ~35 registers and their constants.)
  int stop = kept;
  double carry = 1.0;
  for (int i0 = 0; i0 < kept && stop == kept; i0 += 64) {
    const int i = i0 + lane;
    double p = 0.0;
    bool odd = false;
    if (i < kept) {
      const float v = sidx ? x[sidx[i]] : x[i];  // (sidx == nullptr: x[] already holds the kept values, best first)
      odd = !(v <= 80.0f) || (!a.log_input && v < 0.0f);  // (outside expf_core_f64's range, a NaN, a negative probability)
      p = a.log_input ? ctcmath::expf_core_f64(odd ? 0.0f : v, tbl) : (double)v;
    }
    const double sum = carry + wave_scan_f64_sum(p);
    const bool near = i < kept && (odd || fabs(sum - a.cut_exp) <= 1e-8 * a.cut_exp || !(sum == sum));
    const bool hit = i < kept && (sum >= a.cut_exp || i + 1 >= a.top_n);
    const unsigned long long mh = __ballot(hit), mn = __ballot(near);
    const int firsthit = mh ? __ffsll((long long)mh) - 1 : 64;
    if (mn && (__ffsll((long long)mn) - 1) <= firsthit) flag = true;
    if (mh) stop = i0 + firsthit + 1;
    carry = f64_from_lane(sum, 63);
  }
  flag = __ballot(flag) != 0ull;
  return stop;
}

// The kept length of a frame ranked by one of the workgroup kernels (wave 0), for half rows with equal values inside cutoff_top_n
// (prune_rows_kernel says why this is exact): the cut walks the distinct values before the first such group only, and the frame is
// flagged unless it stops there.  Every lane of the wave passes its own (tie, first_tie).
__device__ __forceinline__ int prune_half_tie_cut(const PruneArgs &a, const float *sval, int kept, int lane, bool &flag, bool tie, int first_tie,
                                                  const uint64_t *tbl) {
  tie = __ballot(tie) != 0ull;
  if (!tie || flag) {
    flag = flag || tie;
    return a.cutoff_prob < 1.0 && !flag ? prune_cumulative_cut(a, sval, nullptr, kept, lane, flag, tbl) : kept;
  }
  if (!(a.cutoff_prob < 1.0)) { flag = true; return kept; }
  // the walk goes through the first tied position as well (sval holds the group's common value there -- or, where a listed label may
  // tie an unlisted one, a value that can only delay a stop past first_tie): a cut that stops at or before first_tie settles the frame,
  // one that reaches first_tie + 1 or runs on leaves it to prune_resolve_kernel.  (first_tie < kept: it is the rank of a kept label.)
  const int ft = wave_min(first_tie);
  const int len = prune_cumulative_cut(a, sval, nullptr, ft + 1, lane, flag, tbl);
  if (len > ft) flag = true;
  return len;
}

// (workgroups per CU: the pass is bound by the latency chain of a frame inside a workgroup, so what counts is how many frames a CU
//  has in flight.  Rounds 2-5, with the device library's exp / log in the cumulative cut (88 VGPRs at the compiler's own choice):
//  0.418 ms at five, 0.349 at six, 0.39 / 0.43 at seven / eight, where the register budget cost more than the extra frames brought.
//  Round 6, without them (63 VGPRs): 0.354 ms at six, 0.336 at seven, 0.323 at eight -- profiles/r06i_prune_variants.txt)
#ifndef CTC_PRUNE_WG_OCC
#define CTC_PRUNE_WG_OCC 8
#endif
// REG (round 6, late): the row stays in registers between the two looks at it (4 * F4 VGPRs; fewer workgroups per CU) instead of
// being read again -- the second sweep fetched four lines in five once more (a line serves eight threads, one thread in five
// looks again): counter traffic 1.78x the row.
#ifndef CTC_PRUNE_REG_OCC
#define CTC_PRUNE_REG_OCC 5
#endif
template <int F4, bool REG, int DT>
__global__ void __launch_bounds__(256, REG ? (F4 <= 4 ? 8 : F4 <= 10 ? CTC_PRUNE_REG_OCC : 3) : CTC_PRUNE_WG_OCC) prune_rows_wg_kernel(PruneArgs a) {
  const typename InElem<DT>::T *in = in_rows<DT>(a.in);
  extern __shared__ __attribute__((aligned(16))) char psm[];
  __shared__ uint32_t s_bound[4];
  __shared__ int s_cnt;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.top_n < a.V ? a.top_n : a.V;
  const int nq = (n + 3) >> 2;  // per-wave share
  // LDS: the kept values in final order (for the cumulative cut) | spare | (unused) | candidate keys | their labels | their values
  float *sval = (float *)psm;
  uint32_t *ckey = (uint32_t *)(sval + ((3 * a.stride + 3) & ~3));  // (16-byte aligned: read four keys at a time)
  int *cidx = (int *)ckey + kPruneCand;
  float *cval = (float *)(cidx + kPruneCand);
  const int nv4 = a.V >> 2;
  constexpr int kChunk = F4 < 5 ? F4 : 5;  // 128-bit loads in flight per thread (measured: 2, 4 and 10 are slower)
  for (long long r = blockIdx.x; r < a.rows; r += gridDim.x) {
    if (a.seq_lens) {
      const long long b = r / a.T;
      int len = a.seq_lens[b];
      len = len < 0 ? 0 : len;
      if ((int)(r - b * a.T) >= len) continue;
    }
    const typename InElem<DT>::T *x4 = in + (size_t)r * a.V;
    if (tid == 0) s_cnt = 0;
    uint32_t lmax = 0;
    float4 vr[REG ? F4 : 1];
    int tq = tid;
    if (REG) {
      asm volatile("" : "+v"(tq));  // (opaque per frame: prune_logits_wg_kernel says why)
#pragma unroll
      for (int u = 0; u < F4; ++u) {
        const int i4 = tq + 256 * u;
        vr[u] = i4 < nv4 ? in_load4<DT>(x4, i4) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      }
#pragma unroll
      for (int u = 0; u < F4; ++u) {
        const int i4 = tq + 256 * u;
        if (i4 < nv4) {
          const uint32_t k0 = prune_key(vr[u].x), k1 = prune_key(vr[u].y), k2 = prune_key(vr[u].z), k3 = prune_key(vr[u].w);
          const uint32_t m01 = k0 > k1 ? k0 : k1, m23 = k2 > k3 ? k2 : k3, m = m01 > m23 ? m01 : m23;
          lmax = m > lmax ? m : lmax;
        }
      }
    }
    for (int u0 = 0; !REG && u0 < F4; u0 += kChunk) {
      float4 v[kChunk];
#pragma unroll
      for (int u = 0; u < kChunk; ++u) {
        const int i4 = tid + 256 * (u0 + u);
        v[u] = (u0 + u < F4 && i4 < nv4) ? in_load4<DT>(x4, i4) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
      }
#pragma unroll
      for (int u = 0; u < kChunk; ++u) {
        const int i4 = tid + 256 * (u0 + u);
        if (u0 + u < F4 && i4 < nv4) {
          const uint32_t k0 = prune_key(v[u].x), k1 = prune_key(v[u].y), k2 = prune_key(v[u].z), k3 = prune_key(v[u].w);
          const uint32_t m01 = k0 > k1 ? k0 : k1, m23 = k2 > k3 ? k2 : k3, m = m01 > m23 ? m01 : m23;
          lmax = m > lmax ? m : lmax;
        }
      }
    }
    uint32_t bw = 0;
    for (int bit = 31; bit >= 12; --bit) {
      const uint32_t trial = bw | (1u << bit);
      if (__popcll(__ballot(lmax >= trial)) >= nq) bw = trial;
    }
    if (lane == 0) s_bound[wave] = bw;
    __syncthreads();
    uint32_t bound = s_bound[0];
    bound = s_bound[1] < bound ? s_bound[1] : bound;
    bound = s_bound[2] < bound ? s_bound[2] : bound;
    bound = s_bound[3] < bound ? s_bound[3] : bound;
    if (REG) {
      if (lmax >= bound && lmax != 0u) {
#pragma unroll
        for (int u = 0; u < F4; ++u) {
          const int i4 = tq + 256 * u;
          if (i4 < nv4) {
            const float4 v = vr[u];
            const uint32_t kk[4] = {prune_key(v.x), prune_key(v.y), prune_key(v.z), prune_key(v.w)};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (kk[e] >= bound && kk[e] != 0u) {
                const int p = atomicAdd(&s_cnt, 1);
                if (p < kPruneCand) { ckey[p] = kk[e]; cidx[p] = 4 * i4 + e; cval[p] = e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
              }
          }
        }
      }
    } else if (lmax >= bound && lmax != 0u) {  // (only the few threads that hold a value at or above the bound sweep again)
      for (int u = 0; u < F4; ++u) {
        const int i4 = tid + 256 * u;
        if (i4 >= nv4) break;
        const float4 v = in_load4<DT>(x4, i4);
        const uint32_t kk[4] = {prune_key(v.x), prune_key(v.y), prune_key(v.z), prune_key(v.w)};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (kk[e] >= bound && kk[e] != 0u) {
            const int p = atomicAdd(&s_cnt, 1);
            if (p < kPruneCand) { ckey[p] = kk[e]; cidx[p] = 4 * i4 + e; cval[p] = e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
          }
      }
    }
    __syncthreads();
    const int ns = s_cnt;
    if (wave == 0) {
      bool flag = ns > kPruneCand;  // more values above the bound than the list holds: prune_resolve_kernel decides this frame
      bool tie = false;     // (half rows: prune_half_tie_cut)
      int first_tie = n;
      int kept = 0;
      int *och = a.ch + (size_t)r * a.stride;
      float *olp = a.lp + (size_t)r * a.stride;
      if (!flag) {
        // every lane ranks its own candidates among all of them: rank = #greater; the n-th largest has rank < n <= rank + #equal
        // (everything this wave needs from here on sits in LDS -- the other three waves of the workgroup wait for it, so a
        //  global access or a chain of dependent LDS reads here is paid by the whole row: the keys are read four at a
        //  time, the values come from the list the second sweep filled)
        for (int p = ns + lane; p < ((ns + 3) & ~3); p += 64) ckey[p] = 0u;  // pad to a multiple of four, below every real key
        __builtin_amdgcn_s_waitcnt(0xc07f);
        for (int q0 = 0; q0 < ns; q0 += 64) {
          const int q = q0 + lane;
          const uint32_t mine = q < ns ? ckey[q] : 0xFFFFFFFFu;
          int gg = 0, ee = 0;
          for (int o = 0; o < ns; o += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4 *>(ckey + o);
            gg += (k4.x > mine) + (k4.y > mine) + (k4.z > mine) + (k4.w > mine);
            ee += (k4.x == mine) + (k4.y == mine) + (k4.z == mine) + (k4.w == mine);
          }
          const bool keep = q < ns && gg < n;
          if constexpr (DT == kInF32) {
            if (keep && gg + ee > n) flag = true;   // equal values straddle the cut: std::sort decides which of them are kept
            if (keep && ee > 1) flag = true;        // equal kept values: their order is std::sort's business
          } else if (keep && ee > 1) {  // (a straddling group has ee > 1; every member writes the group's value: prune_half_tie_cut reads it)
            tie = true; first_tie = gg < first_tie ? gg : first_tie;
            sval[gg] = cval[q];
          }
          if (keep && ee == 1) {
            const int idx = cidx[q];
            float v = cval[q];
            if (!a.log_input) {  // decoder_utils.cpp:42
              v = (float)ctcmath::log_f64((double)v + (double)FLT_MIN, g_t64);
            }
            och[gg] = idx; olp[gg] = v; sval[gg] = cval[q];  // (sval: the row's own value, before any prob -> log conversion)
          }
          kept += __popcll(__ballot(keep));
        }
        if (kept > n) kept = n;
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS writes are visible to its other lanes
      flag = __ballot(flag) != 0ull;
      int len = kept;
      if constexpr (DT == kInF32) {
        if (a.cutoff_prob < 1.0 && !flag) len = prune_cumulative_cut(a, sval, nullptr, kept, lane, flag, a.tables);
      } else {
        len = prune_half_tie_cut(a, sval, kept, lane, flag, tie, first_tie, a.tables);
      }
      if (lane == 0) {
        a.cnt[r] = len;
        if (flag) {
          const unsigned k = atomicAdd(a.n_flag, 1u);
          if (k < a.flag_cap) a.flag_rows[k] = (unsigned)r;
        }
      }
    }
    __syncthreads();  // the lists are reused by the next frame
  }
}

// Raw logits (log_input == 2) straight into the prune: the frame's log-softmax is never written.  One workgroup per frame as
// above, but the row -- read once, 128-bit loads -- stays in registers: its maximum and the lower bound of the n-th largest
// logit come from the first look at it, the sum of exponentials in the order ctcd_log_softmax defines from wg_exp_sum, and only
// the few dozen labels at or above the bound are ever normalised: y = (x - m) - ls, ranked on y (two logits can round to one y).
// x -> y is monotone, so a label below the bound cannot outrank one above it; it could TIE with the n-th largest y if that
// equals the bound's own image -- such a frame is flagged, as are frames that hold a NaN or +inf (no order argument there), and
// prune_resolve_kernel settles flagged frames from the logits with the frame's (m, ls) stored here.
// Requires V % 4 == 0, V <= 1024 * F4, cutoff_top_n <= 64.
__device__ __forceinline__ float prune_key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
#ifndef CTC_PRUNE_LOGITS_OCC
#define CTC_PRUNE_LOGITS_OCC 5
#endif
template <int F4, int DT>
__global__ void __launch_bounds__(256, F4 <= 4 ? 6 : F4 <= 10 ? CTC_PRUNE_LOGITS_OCC : 3) prune_logits_wg_kernel(PruneArgs a, const uint64_t *tables) {
  const typename InElem<DT>::T *in = in_rows<DT>(a.in);
  extern __shared__ __attribute__((aligned(16))) char psm[];
  __shared__ uint64_t tbl[64];
  __shared__ __attribute__((aligned(16))) LsmLds s;
  __shared__ uint32_t s_bound[4];
  __shared__ int s_cnt;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.top_n < a.V ? a.top_n : a.V;
  const int nq = (n + 3) >> 2;  // per-wave share
  float *sval = (float *)psm;
  uint32_t *ckey = (uint32_t *)(sval + ((3 * a.stride + 3) & ~3));
  int *cidx = (int *)ckey + kPruneCand;
  float *cval = (float *)(cidx + kPruneCand);
  const int nv4 = a.V >> 2;
  if (tid < 64) tbl[tid] = tables[tid];
  __syncthreads();
  for (long long r = blockIdx.x; r < a.rows; r += gridDim.x) {
    if (a.seq_lens) {
      const long long b = r / a.T;
      int len = a.seq_lens[b];
      len = len < 0 ? 0 : len;
      if ((int)(r - b * a.T) >= len) continue;
    }
    const typename InElem<DT>::T *x4 = in + (size_t)r * a.V;
    // (the thread index, opaque per frame: derived from the hoisted one, every chunk's predicate and offsets would be kept in
    //  registers across the frame loop -- thirty-odd of them, spilled)
    int tq = tid;
    asm volatile("" : "+v"(tq));
    float4 v[F4];
#pragma unroll
    for (int u = 0; u < F4; ++u) {
      const int i4 = tq + 256 * u;
      v[u] = i4 < nv4 ? in_load4<DT>(x4, i4) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    }
    if (tid == 0) s_cnt = 0;
    // (maxima on the values themselves -- a NaN is skipped, as by the one-wave kernel; the key of the thread's maximum is the
    //  maximum of its keys whenever the row holds no NaN, and rows that do are flagged below)
    float mine = -INFINITY;
#pragma unroll
    for (int u = 0; u < F4; ++u) mine = fmaxf(fmaxf(fmaxf(mine, v[u].x), fmaxf(v[u].y, v[u].z)), v[u].w);
    const uint32_t lmax = prune_key(mine);
    uint32_t bw = 0;
    for (int bit = 31; bit >= 12; --bit) {
      const uint32_t trial = bw | (1u << bit);
      if (__popcll(__ballot(lmax >= trial)) >= nq) bw = trial;
    }
    if (lane == 0) s_bound[wave] = bw;
    const float m = wg_row_max(mine, s, tid);  // (contains a barrier: s_bound is in place)
    uint32_t bound = s_bound[0];
    bound = s_bound[1] < bound ? s_bound[1] : bound;
    bound = s_bound[2] < bound ? s_bound[2] : bound;
    bound = s_bound[3] < bound ? s_bound[3] : bound;
    float ls = 0.0f;
    bool rowflag = !(m > -INFINITY);
    if (!rowflag) {
      const float sum = wg_exp_sum<F4>(v, nv4, m, s, tbl, tq);
      rowflag = !(sum == sum);  // a NaN or +inf among the logits: (x - m) is a NaN for it, and so is the sum
      ls = ctcmath::logf_normal(sum, tbl);
    }
    if (tid == 0) { a.row_max[r] = m; a.row_lse[r] = ls; }
    // the labels at or above the bound, compared as values: for numbers, x >= value(bound) <=> key(x) >= bound (the key is monotone
    // and value(bound)'s key is bound itself); a bound below every number's key decodes to a NaN pattern: everything is listed
    const float bf = prune_key_value(bound);
    const bool all = bound <= prune_key(-INFINITY);
    if (!rowflag && (all || mine >= bf)) {
#pragma unroll
      for (int u = 0; u < F4; ++u) {
        const int i4 = tq + 256 * u;
        if (i4 < nv4) {
          const float xs[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (all || xs[e] >= bf) {
              const int p = atomicAdd(&s_cnt, 1);
              if (p < kPruneCand) { const float y = (xs[e] - m) - ls; ckey[p] = prune_key(y); cidx[p] = 4 * i4 + e; cval[p] = y; }
            }
          }
        }
      }
    }
    __syncthreads();
    const int ns = s_cnt;
    if (wave == 0) {
      bool flag = rowflag || ns > kPruneCand;
      bool tie = false;     // (half rows: prune_half_tie_cut)
      int first_tie = n;
      int kept = 0;
      int *och = a.ch + (size_t)r * a.stride;
      float *olp = a.lp + (size_t)r * a.stride;
      if (!flag) {
        // the image of the bound: no label outside the list has a larger y
        const uint32_t ybkey = bound ? prune_key((prune_key_value(bound) - m) - ls) : 0u;
        for (int p = ns + lane; p < ((ns + 3) & ~3); p += 64) ckey[p] = 0u;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        for (int q0 = 0; q0 < ns; q0 += 64) {
          const int q = q0 + lane;
          const uint32_t mine_k = q < ns ? ckey[q] : 0xFFFFFFFFu;
          int gg = 0, ee = 0;
          for (int o = 0; o < ns; o += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4 *>(ckey + o);
            gg += (k4.x > mine_k) + (k4.y > mine_k) + (k4.z > mine_k) + (k4.w > mine_k);
            ee += (k4.x == mine_k) + (k4.y == mine_k) + (k4.z == mine_k) + (k4.w == mine_k);
          }
          const bool keep = q < ns && gg < n;
          if constexpr (DT == kInF32) {
            if (keep && gg + ee > n) flag = true;   // equal values straddle the cut: std::sort decides which of them are kept
            if (keep && ee > 1) flag = true;        // equal kept values: their order is std::sort's business
            if (keep && mine_k <= ybkey) flag = true;  // a label outside the list could tie with this one
          } else if (keep && (ee > 1 || mine_k <= ybkey)) {
            // (a label outside the list that could tie with this one: a group that may begin at gg -- and unlisted labels that rank
            //  above it may exist too: positions from gg on are uncertain, the ones before it exact)
            tie = true; first_tie = gg < first_tie ? gg : first_tie;
            sval[gg] = cval[q];
          }
          if (keep && ee == 1) { och[gg] = cidx[q]; olp[gg] = cval[q]; sval[gg] = cval[q]; }
          kept += __popcll(__ballot(keep));
        }
        if (kept > n) kept = n;
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      flag = __ballot(flag) != 0ull;
      int len = kept;
      if constexpr (DT == kInF32) {
        if (a.cutoff_prob < 1.0 && !flag) len = prune_cumulative_cut(a, sval, nullptr, kept, lane, flag, tbl);
      } else {
        len = prune_half_tie_cut(a, sval, kept, lane, flag, tie, first_tie, tbl);
      }
      if (lane == 0) {
        a.cnt[r] = len;
        if (flag) {
          const unsigned k = atomicAdd(a.n_flag, 1u);
          if (k < a.flag_cap) a.flag_rows[k] = (unsigned)r;
        }
      }
    }
    __syncthreads();  // the lists are reused by the next frame
  }
}

// Flagged frames are settled here, on the device.  Most flags are ties: equal values at or above the cut, whose order (and,
// at the cut, which of them are kept) is whatever std::sort leaves behind -- a function of the whole row.  One workgroup
// per flagged frame replays that std::sort call (decoder_utils.cpp:19-20: (index, double) pairs in index order, compared
// on the value alone) with stl_emul.h's workgroup-parallel introsort, takes the first min(top_n, V) pairs, converts them
// with the bit-exact binary64 log and walks the cumulative cut as the reference does: a sequential chain of
// log_sum_exp<double> (prune_exact_cut).  Nothing is left for the host (rounds 1-3 sent borderline libm roundings, NaN rows
// and rows too long for the workgroup's LDS there: the first are exact now, the second defined -- prune_key --, the third
// sort in a per-workgroup block of global memory, slowly).
struct WgSortX {
  uint32_t *wsum;  // one word per wave (shared)
  // exclusive prefix (in thread order) and total of one word per thread; contains a barrier
  __device__ __forceinline__ int lanes() const { return 64; }
  __device__ __forceinline__ uint64_t ballot(bool p) const { return __builtin_amdgcn_ballot_w64(p); }
  __device__ __forceinline__ int count(uint64_t m) const { return __builtin_popcountll(m); }
  __device__ __forceinline__ int count_below(uint64_t m) const { return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }
  __device__ __forceinline__ uint32_t first_lane(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
  __device__ __forceinline__ void block_scan_u32(uint32_t mine, uint32_t *base_out, uint32_t *total_out) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6, nw = ((int)blockDim.x + 63) >> 6;
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int q = 0; q < nw; ++q) { const uint32_t t = wsum[q]; if (q < wave) base += t; tot += t; }
    *base_out = base + incl - mine;
    *total_out = tot;
    __syncthreads();  // (wsum is reused by the next round)
  }
  __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int nt() const { return (int)blockDim.x; }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ int atomic_add(int *p, int v) { return atomicAdd(p, v); }
  __device__ __forceinline__ int uni(int v) const { return __builtin_amdgcn_readfirstlane(v); }
};
// (prune_resolve_task_cap, kResolveThreads, kResolveMaxV and prune_resolve_lds_bytes: prepass.h)
constexpr int kResolveBigCut = 256;    // ranges longer than this are split by the whole workgroup
// decoder_utils.cpp:25-32 to the letter, by one thread: cum = log_sum_exp<double>(cum, log p_i) from cum = 0.0 over the sorted
// candidates until cum >= cutoff_prob or cutoff_top_n of them are taken; every log / exp the bit-exact one.
template <int DT>
__device__ int prune_exact_cut(const PruneArgs &a, const typename InElem<DT>::T *row, const int *sidx, int n, float m, float ls) {
  double cum = 0.0;
  int keep = 0;
  for (int i = 0; i < n; ++i) {
    const double v = (double)prune_row_value(a, in_at<DT>(row, sidx[i]), m, ls);
    cum = ctcmath::lse_f64(cum, a.log_input ? v : ctcmath::log_f64(v, g_t64), g_t64);
    ++keep;
    if (cum >= a.cutoff_prob || keep >= a.top_n) break;
  }
  return keep;
}

// far != nullptr: the sort's arrays do not fit the workgroup's LDS (vocabularies beyond ~11 000 labels): they live in a block
// of global memory per workgroup (far_stride bytes each; every barrier of the sort is a full fence already).
template <int DT>
__global__ void __launch_bounds__(kResolveThreads) prune_resolve_kernel(PruneArgs a, char *far, size_t far_stride) {
  extern __shared__ __attribute__((aligned(16))) char rsm_lds[];
  __shared__ uint32_t s_wsum[kResolveThreads / 64];
  char *rsm = far ? far + (size_t)blockIdx.x * far_stride : rsm_lds;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int V = a.V, n = a.top_n < V ? a.top_n : V;
  const int tcap = prune_resolve_task_cap(V);
  unsigned long long *v = (unsigned long long *)rsm;
  uint16_t *Lp = (uint16_t *)(v + V), *Rp = Lp + (V + 2), *cur = Rp + (V + 2), *nxt = cur + 3 * tcap, *small = nxt + 3 * tcap;
  int *bstack = (int *)(((uintptr_t)(small + 2 * (V / 2 + 1)) + 15) & ~(uintptr_t)15);
  int *cnt = bstack + 3 * 64, *sidx = cnt + 4;
  const unsigned raw = *a.n_flag, nf = raw < a.flag_cap ? raw : a.flag_cap;
  WgSortX x{s_wsum};
  for (unsigned k = blockIdx.x; k < nf; k += gridDim.x) {
    const long long r = (long long)a.flag_rows[k];
    const typename InElem<DT>::T *row = in_rows<DT>(a.in) + (size_t)r * V;
    const float m = a.log_input == 2 ? a.row_max[r] : 0.0f, ls = a.log_input == 2 ? a.row_lse[r] : 0.0f;  // (raw logits: prune_logits_wg_kernel)
    __syncthreads();
    for (int i = tid; i < V; i += kResolveThreads) v[i] = ((unsigned long long)prune_key(prune_row_value(a, in_at<DT>(row, i), m, ls)) << 32) | (unsigned)i;
    __syncthreads();
    // decoder_utils.cpp:19-20: (index, double) pairs in index order, std::sort on the value alone, descending
    // (stl_emul.h: long ranges split by the whole workgroup, the rest by one thread per range; only the ranges that reach
    //  the first n places -- the prune pass keeps the best top_n of a row)
    stlemu::sort_prefix_parallel(x, v, V, n, kResolveBigCut, [](unsigned long long e) { return (uint32_t)(e >> 32); }, Lp, Rp, cur, nxt, small,
                                 cnt, bstack);
    if (tid < 64) {
      int *och = a.ch + (size_t)r * a.stride;
      float *olp = a.lp + (size_t)r * a.stride;
      for (int q = lane; q < n; q += 64) {
        const int idx = (int)(uint32_t)v[q];
        float val = prune_row_value(a, in_at<DT>(row, idx), m, ls);
        if (!a.log_input) val = (float)ctcmath::log_f64((double)val + (double)FLT_MIN, g_t64);  // decoder_utils.cpp:42
        och[q] = idx; olp[q] = val; sidx[q] = idx;
      }
      __threadfence_block();  // the wave's own writes (LDS or global) are visible to its lane 0
      if (lane == 0) a.cnt[r] = a.cutoff_prob < 1.0 ? prune_exact_cut<DT>(a, row, sidx, n, m, ls) : n;
    }
  }
}

// ---- launch order (ctcd_set_launch_order): the permutation the decode kernel's workgroups take their items from by ticket
// (decode_kernel.h KernelArgs::order = [ticket | permutation]), longest utterance first, ties in batch order -- a pure function of
// the clamped lengths.  Either kernel also zeroes the ticket counter (order[0]) of the launch behind it.
__device__ __forceinline__ int order_len(const int32_t *lens, int i, int T) {
  const int l = lens ? lens[i] : T;
  return l < 0 ? 0 : (l > T ? T : l);  // (as the decode kernel clamps them: binding.cpp:64-65)
}

// B <= kOrderSortMax: one workgroup sorts the keys (T - len) << 32 | b -- unique, so the sort is stable by construction -- with a
// bitonic network in LDS; n = B rounded up to a power of two (the padding keys sort last).
__global__ void __launch_bounds__(kOrderThreads) launch_order_sort_kernel(const int32_t *lens, int B, int T, int n, int *order) {
  extern __shared__ unsigned long long okey[];
  for (int i = threadIdx.x; i < n; i += blockDim.x)
    okey[i] = i < B ? ((unsigned long long)(unsigned)(T - order_len(lens, i, T)) << 32) | (unsigned)i : ~0ull;
  if (threadIdx.x == 0) order[0] = 0;
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (n >> 1); i += blockDim.x) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;  // (pair i of the stage: bit log2(j) of lo is 0)
        const unsigned long long x = okey[lo], y = okey[hi];
        if ((x > y) == ((lo & k) == 0)) { okey[lo] = y; okey[hi] = x; }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < B; i += blockDim.x) order[1 + i] = (int)(unsigned)okey[i];
}

// Larger batches: every item counts the items that go in front of it and writes itself to its rank.  O(B^2) compares spread over
// ceil(B / 256) workgroups: 0.52 ms at B = 20000, growing with the square (about 50 ms at 200 000 items, a second near a million --
// where the decode itself takes far longer still).
constexpr int kOrderRankTile = 1024;  // (kOrderThreads, kOrderSortMax, kOrderRankThreads: prepass.h)
__global__ void __launch_bounds__(kOrderRankThreads) launch_order_rank_kernel(const int32_t *lens, int B, int T, int *order) {
  __shared__ int tile[kOrderRankTile];
  const int i = blockIdx.x * kOrderRankThreads + threadIdx.x;
  const int li = i < B ? order_len(lens, i, T) : 0;
  int rank = 0;
  for (int j0 = 0; j0 < B; j0 += kOrderRankTile) {
    __syncthreads();
    for (int t = threadIdx.x; t < kOrderRankTile; t += kOrderRankThreads) tile[t] = j0 + t < B ? order_len(lens, j0 + t, T) : -1;
    __syncthreads();
    for (int t = 0; t < kOrderRankTile; ++t) {
      const int lj = tile[t];  // (-1 past the end: never in front)
      rank += lj > li || (lj == li && j0 + t < i);
    }
  }
  if (i < B) order[1 + rank] = i;
  if (i == 0) order[0] = 0;
}

}  // namespace

namespace ctcprepass {

#define CTC_PP(K, A, B, DT, VMAX, ...) {(const void *)__VA_ARGS__, K, A, B, DT, VMAX}
#define CTC_PP_DT(DT)                                                                                                                    \
  CTC_PP(CTCD_PP_PROB_TO_LOG, 0, 0, DT, 0, prob_to_log_kernel<DT>), CTC_PP(CTCD_PP_LSM_WAVE, 0, 0, DT, 0, log_softmax_rows_kernel<DT>),  \
  CTC_PP(CTCD_PP_LSM_WG, 1, 0, DT, 1024, log_softmax_rows_wg_kernel<1, DT>), CTC_PP(CTCD_PP_LSM_WG, 2, 0, DT, 2048, log_softmax_rows_wg_kernel<2, DT>), \
  CTC_PP(CTCD_PP_LSM_WG, 4, 0, DT, 4096, log_softmax_rows_wg_kernel<4, DT>), CTC_PP(CTCD_PP_LSM_WG, 10, 0, DT, 10240, log_softmax_rows_wg_kernel<10, DT>), \
  CTC_PP(CTCD_PP_LSM_WG, 16, 0, DT, 0, log_softmax_rows_wg_kernel<16, DT>),                                                              \
  CTC_PP(CTCD_PP_PRUNE_ROWS, 1, 0, DT, 64, prune_rows_kernel<1, DT>), CTC_PP(CTCD_PP_PRUNE_ROWS, 4, 0, DT, 256, prune_rows_kernel<4, DT>),   \
  CTC_PP(CTCD_PP_PRUNE_ROWS, 16, 0, DT, 1024, prune_rows_kernel<16, DT>), CTC_PP(CTCD_PP_PRUNE_ROWS, 64, 0, DT, 4096, prune_rows_kernel<64, DT>), \
  CTC_PP(CTCD_PP_PRUNE_ROWS, 160, 0, DT, 10240, prune_rows_kernel<160, DT>), CTC_PP(CTCD_PP_PRUNE_ROWS, 0, 0, DT, 0, prune_rows_kernel<0, DT>), \
  CTC_PP(CTCD_PP_PRUNE_WG, 1, 0, DT, 1024, prune_rows_wg_kernel<1, false, DT>), CTC_PP(CTCD_PP_PRUNE_WG, 2, 0, DT, 2048, prune_rows_wg_kernel<2, false, DT>), \
  CTC_PP(CTCD_PP_PRUNE_WG, 4, 0, DT, 4096, prune_rows_wg_kernel<4, false, DT>), CTC_PP(CTCD_PP_PRUNE_WG, 10, 0, DT, 10240, prune_rows_wg_kernel<10, false, DT>), \
  CTC_PP(CTCD_PP_PRUNE_WG, 16, 0, DT, 0, prune_rows_wg_kernel<16, false, DT>),                                                           \
  /* (the row held in registers between the two looks at it: V <= 10240; beyond, the registers run out) */                              \
  CTC_PP(CTCD_PP_PRUNE_WG, 1, 1, DT, 1024, prune_rows_wg_kernel<1, true, DT>), CTC_PP(CTCD_PP_PRUNE_WG, 2, 1, DT, 2048, prune_rows_wg_kernel<2, true, DT>), \
  CTC_PP(CTCD_PP_PRUNE_WG, 4, 1, DT, 4096, prune_rows_wg_kernel<4, true, DT>), CTC_PP(CTCD_PP_PRUNE_WG, 10, 1, DT, 10240, prune_rows_wg_kernel<10, true, DT>), \
  CTC_PP(CTCD_PP_PRUNE_LOGITS, 1, 0, DT, 1024, prune_logits_wg_kernel<1, DT>), CTC_PP(CTCD_PP_PRUNE_LOGITS, 2, 0, DT, 2048, prune_logits_wg_kernel<2, DT>), \
  CTC_PP(CTCD_PP_PRUNE_LOGITS, 4, 0, DT, 4096, prune_logits_wg_kernel<4, DT>), CTC_PP(CTCD_PP_PRUNE_LOGITS, 10, 0, DT, 10240, prune_logits_wg_kernel<10, DT>), \
  CTC_PP(CTCD_PP_PRUNE_LOGITS, 16, 0, DT, 0, prune_logits_wg_kernel<16, DT>), CTC_PP(CTCD_PP_RESOLVE, 0, 0, DT, 0, prune_resolve_kernel<DT>)
const PrepassEntry kPrepass[] = {
  CTC_PP_DT(kInF32), CTC_PP_DT(kInF16), CTC_PP_DT(kInBF16),
  CTC_PP(CTCD_PP_WIDEN, 0, 0, kInF16, 0, widen_rows_kernel<kInF16>), CTC_PP(CTCD_PP_WIDEN, 0, 0, kInBF16, 0, widen_rows_kernel<kInBF16>),
};
#undef CTC_PP_DT
#undef CTC_PP
const int kPrepassCount = (int)(sizeof(kPrepass) / sizeof(kPrepass[0]));
const PrepassEntry *pp_pick(int k, int b, int dt, int V) {
  for (const PrepassEntry &e : kPrepass)
    if (e.kernel == k && e.b == b && e.dt == dt && (e.vmax == 0 || V <= e.vmax)) return &e;
  return nullptr;
}
const PrepassEntry *pp_find(const void *fn) {
  for (const PrepassEntry &e : kPrepass)
    if (e.fn == fn) return &e;
  return nullptr;
}

hipError_t launch_order(const int32_t *lens, int B, int T, int max_lds, int *order, hipStream_t stream) {
  int n = 1;
  while (n < B) n <<= 1;
  if (B <= kOrderSortMax && (size_t)n * 8 <= (size_t)max_lds) {
    const hipError_t e = hipFuncSetAttribute((const void *)launch_order_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, n * 8);
    if (e != hipSuccess) return e;
    launch_order_sort_kernel<<<1, kOrderThreads, (size_t)n * 8, stream>>>(lens, B, T, n, order);
  } else {
    launch_order_rank_kernel<<<(B + kOrderRankThreads - 1) / kOrderRankThreads, kOrderRankThreads, 0, stream>>>(lens, B, T, order);
  }
  return hipGetLastError();
}

}  // namespace ctcprepass
