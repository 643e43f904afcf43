// lsm_device.h -- the workgroup helpers that give a long row's log-softmax the summation order ctcd_log_softmax defines
// (include/ctcdecode_amd.h): the row's maximum and the sum of its exponentials over 64 chains, for a row that a workgroup of four waves
// holds in registers (thread t: the float4s t, t + 256, ...).  Device code with barriers and wave intrinsics, shared by the kernels that
// hold a row that way: log_softmax_rows_wg_kernel and prune_logits_wg_kernel (prepass.hip) and the greedy decode's logit kernel
// (greedy.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "exact_math.h"

namespace ctclsm {

// The sum keeps the order the definition fixes -- 64 chains, chain l over the terms j = l, l + 64, ... in increasing j -- although no
// thread holds a chain's terms: the exponentials of 1024 consecutive labels at a time go to LDS (every thread computes four), and one
// wave per such chunk (the four take turns) extends the 64 chains by sixteen terms each, lane l reading its chain's terms at
// l + 64 k.  Two chunk buffers, one barrier per chunk; the chains' running values pass from wave to wave through LDS.
// Requires V % 4 == 0 and V <= 1024 * F4.
constexpr int kLsmChunk = 1024;  // labels per chunk of exponentials (four per thread)
struct LsmLds {
  float terms[2][kLsmChunk];
  float chain[64];
  float wmax[4];
};
template <int F4>
__device__ __forceinline__ float wg_exp_sum(const float4 (&v)[F4], int nv4, float m, LsmLds &s, const uint64_t *tbl, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int u = 0; u < F4; ++u) {
    if (256 * u < nv4) {  // (uniform; chunks past the row's end would add zeros)
      float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (tid + 256 * u < nv4) {
        // (two at a time: four interleaved binary64 evaluations on top of the row cost registers -- the other waves hide the latency)
        e.x = ctcmath::expf_nonpos(v[u].x - m, tbl); e.y = ctcmath::expf_nonpos(v[u].y - m, tbl);
        __builtin_amdgcn_sched_barrier(0);
        e.z = ctcmath::expf_nonpos(v[u].z - m, tbl); e.w = ctcmath::expf_nonpos(v[u].w - m, tbl);
        __builtin_amdgcn_sched_barrier(0);
      }
      *reinterpret_cast<float4 *>(&s.terms[u & 1][4 * tid]) = e;
      __syncthreads();
      if (wave == (u & 3)) {
        float p = u ? s.chain[lane] : 0.0f;
        const float *c = &s.terms[u & 1][lane];
#pragma unroll
        for (int k = 0; k < kLsmChunk / 64; ++k) p += c[64 * k];
        s.chain[lane] = p;
      }
    }
  }
  __syncthreads();
  float part = s.chain[lane];
  for (int off = 1; off < 64; off <<= 1) part += __shfl_xor(part, off, 64);
  return part;
}
// the row's maximum (NaN-ignoring, as the one-wave kernel's), known to every thread; contains one barrier
__device__ __forceinline__ float wg_row_max(float mine, LsmLds &s, int tid) {
  for (int off = 1; off < 64; off <<= 1) { const float o = __shfl_xor(mine, off, 64); mine = o > mine ? o : mine; }
  if ((tid & 63) == 0) s.wmax[tid >> 6] = mine;
  __syncthreads();
  float m = s.wmax[0];
  m = s.wmax[1] > m ? s.wmax[1] : m; m = s.wmax[2] > m ? s.wmax[2] : m; m = s.wmax[3] > m ? s.wmax[3] : m;
  return m + 0.0f;  // (a zero maximum is +0 whichever zero the reduction met first: part of the definition)
}

}  // namespace ctclsm
