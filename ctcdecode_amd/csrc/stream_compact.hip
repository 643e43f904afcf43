// stream_compact.hip -- the kernels that compact parked streams' node pools (stream_compact.h), one workgroup per stream, no frame
// loop.  A translation unit of its own: the decode kernels (decode_kernels.hip) and the peek (stream_peek.hip) do not see it.
//   ctc_stream_compact_count_kernel   the size of every stream's live set, to page-locked memory (the host sizes the scratch by it)
//   ctc_stream_compact_gather_kernel  the live set in its new layout -> scratch; beam arrays and pool count rewritten in the block
//   ctc_stream_compact_store_kernel   scratch -> the stream's block, or the smaller block it moves to
#include <hip/hip_runtime.h>

#include "stream_compact.h"

namespace ctccompact {

// The workgroup policy of the per-stream routines: plain barriers (every phase reads what another wrote to LDS or to the block).
struct CompactX {
  __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int nt() const { return (int)blockDim.x; }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ int uni(int v) const { return __builtin_amdgcn_readfirstlane(v); }
};

struct CompactArgs {
  CompactCtl ctl;
  int *scratch;
  long long pool_off;
  int K;
};

__global__ void __launch_bounds__(kCompactThreads) ctc_stream_compact_count_kernel(CompactArgs a) {
  extern __shared__ __attribute__((aligned(16))) char compact_smem[];
  const int b = (int)blockIdx.x;
  CompactWork w;
  compact_carve(w, compact_smem, a.K);
  const int *hdr = (const int *)a.ctl.blocks[b];
  CompactX x;
  const CompactPlan pl = compact_plan(x, w, a.K, hdr, hdr + SH_WORDS, a.ctl.pool_caps[b]);
  if (threadIdx.x == 0) a.ctl.live[b] = pl.M;
}

__global__ void __launch_bounds__(kCompactThreads) ctc_stream_compact_gather_kernel(CompactArgs a) {
  extern __shared__ __attribute__((aligned(16))) char compact_smem[];
  const int b = (int)blockIdx.x;
  const int M = a.ctl.live[b];  // (what the count kernel found, and the host cut the scratch for)
  if (M <= 0) return;           // no frames, or a bad state: reported by the count kernel
  CompactWork w;
  compact_carve(w, compact_smem, a.K);
  char *base = a.ctl.blocks[b];
  int *hdr = (int *)base;
  const PoolNode *pool = (const PoolNode *)(base + a.pool_off);
  const int pool_cap = a.ctl.pool_caps[b];
  CompactX x;
  const CompactPlan pl = compact_plan(x, w, a.K, hdr, hdr + SH_WORDS, pool_cap);
  int st = COMPACT_BAD_STATE;
  if (pl.M == M)  // (the parked state the scratch was cut for)
    st = compact_gather(x, w, pl, a.K, hdr, hdr + SH_WORDS, pool, (const int *)(pool + pool_cap), pool_cap, compact_out_at(a.scratch + a.ctl.scr[b], M));
  if (threadIdx.x == 0) a.ctl.status[b] = st;
}

__global__ void __launch_bounds__(kCompactThreads) ctc_stream_compact_store_kernel(CompactArgs a) {
  const int b = (int)blockIdx.x;
  const int M = a.ctl.live[b];
  if (M <= 0 || a.ctl.status[b] != COMPACT_OK) return;  // (a stream the gather refused keeps its block as it is)
  char *src = a.ctl.blocks[b], *dst = a.ctl.dst[b];
  CompactX x;
  compact_write_back(x, M, compact_out_at(a.scratch + a.ctl.scr[b], M), (const int *)src, (int *)dst, (size_t)a.pool_off / sizeof(int),
                     (PoolNode *)(dst + a.pool_off), (int *)((PoolNode *)(dst + a.pool_off) + a.ctl.dst_caps[b]), a.ctl.dst_caps[b]);
}

size_t compact_lds_bytes(int K) {
  CompactWork w;
  return compact_carve(w, nullptr, K);
}

const void *compact_kernel_address(int which) {
  return which == 0 ? (const void *)ctc_stream_compact_count_kernel
                    : which == 1 ? (const void *)ctc_stream_compact_gather_kernel : (const void *)ctc_stream_compact_store_kernel;
}

static CompactArgs compact_args(const CompactLaunch &l) {
  CompactArgs a;
  a.ctl = l.ctl; a.scratch = l.scratch; a.pool_off = l.pool_off; a.K = l.K;
  return a;
}

static int compact_allow_lds(int which, size_t lds) {
  if (lds <= 64 * 1024) return (int)hipSuccess;  // (beams of several thousand entries: more than the default limit of dynamic LDS)
  return (int)hipFuncSetAttribute(compact_kernel_address(which), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

int launch_compact_count(const CompactLaunch &l, void *stream) {
  const size_t lds = compact_lds_bytes(l.K);
  if (const int e = compact_allow_lds(0, lds)) return e;
  hipLaunchKernelGGL(ctc_stream_compact_count_kernel, dim3((unsigned)l.B), dim3(kCompactThreads), lds, (hipStream_t)stream, compact_args(l));
  return (int)hipGetLastError();
}

int launch_compact_move(const CompactLaunch &l, void *stream) {
  const size_t lds = compact_lds_bytes(l.K);
  if (const int e = compact_allow_lds(1, lds)) return e;
  hipLaunchKernelGGL(ctc_stream_compact_gather_kernel, dim3((unsigned)l.B), dim3(kCompactThreads), lds, (hipStream_t)stream, compact_args(l));
  int e = (int)hipGetLastError();
  if (e != (int)hipSuccess) return e;
  hipLaunchKernelGGL(ctc_stream_compact_store_kernel, dim3((unsigned)l.B), dim3(kCompactThreads), 0, (hipStream_t)stream, compact_args(l));
  return (int)hipGetLastError();
}

}  // namespace ctccompact
