// stream_commit.hip -- the kernels that commit parked streams' final labels and drop their trunks (stream_commit.h), one workgroup
// per stream, no frame loop.  A translation unit of its own: the decode kernels (decode_kernels.hip), the peek (stream_peek.hip) and
// the compaction (stream_compact.hip) do not see it.
//   ctc_stream_commit_count_kernel   every stream's live set and drop, to page-locked memory (the host sizes scratch and results by them)
//   ctc_stream_commit_gather_kernel  the live set below the new root -> scratch, the trunk's labels -> scratch; beam arrays (pool
//                                    indices, dep, lcp) and pool count rewritten in the block
//   ctc_stream_commit_store_kernel   scratch -> the stream's block, or the smaller block it moves to
#include <hip/hip_runtime.h>

#include "stream_commit.h"

namespace ctccommit {

// The workgroup policy of the per-stream routines: plain barriers (every phase reads what another wrote to LDS or to the block).
struct CommitX {
  __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int nt() const { return (int)blockDim.x; }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ int uni(int v) const { return __builtin_amdgcn_readfirstlane(v); }
};

struct CommitArgs {
  CommitCtl ctl;
  int *scratch;
  long long pool_off;
  int K;
};

__global__ void __launch_bounds__(kCompactThreads) ctc_stream_commit_count_kernel(CommitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char commit_smem[];
  const int b = (int)blockIdx.x;
  CompactWork w;
  compact_carve(w, commit_smem, a.K);
  const int *hdr = (const int *)a.ctl.c.blocks[b];
  CommitX x;
  const CommitPlan pl = commit_plan(x, w, a.K, hdr, hdr + SH_WORDS, a.ctl.c.pool_caps[b]);
  if (threadIdx.x == 0) { a.ctl.c.live[b] = pl.cp.M; a.ctl.drop[b] = pl.drop; }
}

__global__ void __launch_bounds__(kCompactThreads) ctc_stream_commit_gather_kernel(CommitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char commit_smem[];
  const int b = (int)blockIdx.x;
  const int M = a.ctl.c.live[b], D = a.ctl.drop[b];  // (what the count kernel found, and the host cut the scratch for)
  if (M <= 0) return;                                // no frames, or a bad state: reported by the count kernel
  CompactWork w;
  compact_carve(w, commit_smem, a.K);
  char *base = a.ctl.c.blocks[b];
  int *hdr = (int *)base;
  const PoolNode *pool = (const PoolNode *)(base + a.pool_off);
  const int pool_cap = a.ctl.c.pool_caps[b];
  CommitX x;
  const CommitPlan pl = commit_plan(x, w, a.K, hdr, hdr + SH_WORDS, pool_cap);
  int st = COMPACT_BAD_STATE;
  if (pl.cp.M == M && pl.drop == D && D >= 0 && D < M) {  // (the parked state the scratch was cut for)
    int *lab = a.scratch + a.ctl.lab[b];
    st = commit_gather(x, w, pl, a.K, hdr, hdr + SH_WORDS, pool, (const int *)(pool + pool_cap), pool_cap,
                       compact_out_at(a.scratch + a.ctl.c.scr[b], pl.M), lab, lab + D);
  }
  if (threadIdx.x == 0) a.ctl.c.status[b] = st;
}

__global__ void __launch_bounds__(kCompactThreads) ctc_stream_commit_store_kernel(CommitArgs a) {
  const int b = (int)blockIdx.x;
  const int M = a.ctl.c.live[b] - a.ctl.drop[b];  // nodes of the new layout
  if (a.ctl.c.live[b] <= 0 || M <= 0 || a.ctl.c.status[b] != COMPACT_OK) return;  // (a stream the gather refused keeps its block as it is)
  char *src = a.ctl.c.blocks[b], *dst = a.ctl.c.dst[b];
  CommitX x;
  compact_write_back(x, M, compact_out_at(a.scratch + a.ctl.c.scr[b], M), (const int *)src, (int *)dst, (size_t)a.pool_off / sizeof(int),
                     (PoolNode *)(dst + a.pool_off), (int *)((PoolNode *)(dst + a.pool_off) + a.ctl.c.dst_caps[b]), a.ctl.c.dst_caps[b]);
}

const void *commit_kernel_address(int which) {
  return which == 0 ? (const void *)ctc_stream_commit_count_kernel
                    : which == 1 ? (const void *)ctc_stream_commit_gather_kernel : (const void *)ctc_stream_commit_store_kernel;
}

static CommitArgs commit_args(const CommitLaunch &l) {
  CommitArgs a;
  a.ctl = l.ctl; a.scratch = l.scratch; a.pool_off = l.pool_off; a.K = l.K;
  return a;
}

static int commit_allow_lds(int which, size_t lds) {
  if (lds <= 64 * 1024) return (int)hipSuccess;  // (beams of several thousand entries: more than the default limit of dynamic LDS)
  return (int)hipFuncSetAttribute(commit_kernel_address(which), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

int launch_commit_count(const CommitLaunch &l, void *stream) {
  const size_t lds = compact_lds_bytes(l.K);
  if (const int e = commit_allow_lds(0, lds)) return e;
  hipLaunchKernelGGL(ctc_stream_commit_count_kernel, dim3((unsigned)l.B), dim3(kCompactThreads), lds, (hipStream_t)stream, commit_args(l));
  return (int)hipGetLastError();
}

int launch_commit_move(const CommitLaunch &l, void *stream) {
  const size_t lds = compact_lds_bytes(l.K);
  if (const int e = commit_allow_lds(1, lds)) return e;
  hipLaunchKernelGGL(ctc_stream_commit_gather_kernel, dim3((unsigned)l.B), dim3(kCompactThreads), lds, (hipStream_t)stream, commit_args(l));
  int e = (int)hipGetLastError();
  if (e != (int)hipSuccess) return e;
  hipLaunchKernelGGL(ctc_stream_commit_store_kernel, dim3((unsigned)l.B), dim3(kCompactThreads), 0, (hipStream_t)stream, commit_args(l));
  return (int)hipGetLastError();
}

}  // namespace ctccommit
