// stream_peek.hip -- ctc_stream_peek_kernel: the interim results of live streams (stream_peek.h), one workgroup per stream, no
// frame loop.  A translation unit of its own: the decode kernels (decode_kernels.hip) do not see it.
#include <hip/hip_runtime.h>

#include "stream_peek.h"

namespace ctcpeek {

// The workgroup policy peek_stream needs: plain barriers (every phase reads what another wrote to LDS or to the result rows),
// LDS atomics, a wave as the group.
struct PeekX {
  __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int nt() const { return (int)blockDim.x; }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ int uni(int v) const { return __builtin_amdgcn_readfirstlane(v); }
  __device__ __forceinline__ int atomic_add(int *p, int v) { return atomicAdd(p, v); }
  __device__ __forceinline__ void atomic_min(int *p, int v) { atomicMin(p, v); }
  __device__ __forceinline__ int group() const { return __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6); }
  __device__ __forceinline__ int ngroups() const { return ((int)blockDim.x + 63) >> 6; }
  __device__ __forceinline__ int lane() const { return (int)threadIdx.x & 63; }
  __device__ __forceinline__ int lanes() const { return 64; }
};

struct PeekArgs {
  char *const *blocks;
  const int *pool_caps;
  const int *since;
  long long pool_off;
  int K;
  ctclm::LmView lm;
  PeekOut out;
  int32_t *status;
};

constexpr int kPeekMaxThreads = 256;

template <bool LM>
__global__ void __launch_bounds__(kPeekMaxThreads) ctc_stream_peek_kernel(PeekArgs a) {
  extern __shared__ __attribute__((aligned(16))) char peek_smem[];
  const int b = (int)blockIdx.x;
  PeekWork w;
  peek_carve(w, peek_smem, a.K, LM);
  char *base = a.blocks[b];
  const int *hdr = (const int *)base;
  const PoolNode *pool = (const PoolNode *)(base + a.pool_off);
  const int pool_cap = a.pool_caps[b];
  PeekX x;
  const int st = peek_stream<LM>(x, w, a.K, hdr, hdr + SH_WORDS, pool, (const int *)(pool + pool_cap), pool_cap, &a.lm, a.since[b], a.out, b);
  if (threadIdx.x == 0) a.status[b] = st;
}

template __global__ void ctc_stream_peek_kernel<false>(PeekArgs);
template __global__ void ctc_stream_peek_kernel<true>(PeekArgs);

size_t peek_lds_bytes(int K, bool lm) {
  PeekWork w;
  return peek_carve(w, nullptr, K, lm);
}

// One thread per beam entry up to four waves: the kernel's phases are loops over the K entries (keys, the sorts' ranges, the
// common prefix) or over the segments of the reported rows -- a handful with n_best = 1 -- never over candidate slots, so the
// decode kernels' 1024 threads would idle through every barrier.
int peek_threads(int K) { return K <= 64 ? 64 : K <= 128 ? 128 : kPeekMaxThreads; }

const void *peek_kernel_address(bool lm) {
  return lm ? (const void *)ctc_stream_peek_kernel<true> : (const void *)ctc_stream_peek_kernel<false>;
}

int launch_stream_peek(const PeekLaunch &l, void *stream) {
  PeekArgs a;
  a.blocks = l.blocks; a.pool_caps = l.pool_caps; a.since = l.since; a.pool_off = l.pool_off; a.K = l.K;
  a.lm = ctclm::LmView{};
  if (l.lm) a.lm = *l.lm;
  a.out = l.out;
  a.status = l.status;
  const size_t lds = peek_lds_bytes(l.K, l.lm != nullptr);
  if (lds > 64 * 1024) {  // (beams of several thousand entries: more than the default limit of dynamic LDS)
    const hipError_t e = hipFuncSetAttribute(peek_kernel_address(l.lm != nullptr), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid((unsigned)l.B), block((unsigned)peek_threads(l.K));
  if (l.lm) hipLaunchKernelGGL(ctc_stream_peek_kernel<true>, grid, block, lds, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(ctc_stream_peek_kernel<false>, grid, block, lds, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}

}  // namespace ctcpeek
