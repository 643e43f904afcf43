// stream_snapshot.hip -- the kernels that pack parked streams into images and unpack images into fresh blocks (stream_snapshot.h),
// one workgroup per stream, no frame loop, no dependence on a stream's age.  A translation unit of its own: the decode kernels
// (decode_kernels.hip), the peek, the compaction and the commit do not see it.
//   ctc_stream_export_kernel   a compacted stream's header words, beam arrays and M nodes -> its image in the staging buffer
//   ctc_stream_import_kernel   a validated image in the staging buffer -> a fresh block
#include <hip/hip_runtime.h>

#include "stream_snapshot.h"

namespace ctcsnap {

struct SnapX {
  __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int nt() const { return (int)blockDim.x; }
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ int uni(int v) const { return __builtin_amdgcn_readfirstlane(v); }
};

struct SnapArgs {
  SnapCtl ctl;
  int *staging;
  long long pool_off;
  int K;
};

__global__ void __launch_bounds__(kSnapThreads) ctc_stream_export_kernel(SnapArgs a) {
  const int b = (int)blockIdx.x;
  const char *base = a.ctl.blocks[b];
  const int *hdr = (const int *)base;
  const PoolNode *pool = (const PoolNode *)(base + a.pool_off);
  const int pool_cap = a.ctl.pool_caps[b];
  int M = a.ctl.nodes[b];
  M = M < 1 ? 1 : (M > pool_cap ? pool_cap : M);  // (the image was sized for M nodes; never more than the pool holds)
  SnapX x;
  snapshot_export(x, a.K, M, a.ctl.meta[b], hdr, hdr + SH_WORDS, pool, (const int *)(pool + pool_cap), pool_cap, a.staging + a.ctl.off[b]);
}

__global__ void __launch_bounds__(kSnapThreads) ctc_stream_import_kernel(SnapArgs a) {
  const int b = (int)blockIdx.x;
  char *base = a.ctl.blocks[b];
  const int pool_cap = a.ctl.pool_caps[b];
  const int *img = a.staging + a.ctl.off[b];
  if (img[SN_NODES] > pool_cap || img[SN_BEAM] != a.K) return;  // (the host cut the block for this image)
  PoolNode *pool = (PoolNode *)(base + a.pool_off);
  SnapX x;
  snapshot_import(x, img, (int *)base, (size_t)a.pool_off / sizeof(int), pool, (int *)(pool + pool_cap), pool_cap);
}

const void *snapshot_kernel_address(int which) {
  return which == 0 ? (const void *)ctc_stream_export_kernel : (const void *)ctc_stream_import_kernel;
}

static SnapArgs snap_args(const SnapLaunch &l) {
  SnapArgs a;
  a.ctl = l.ctl; a.staging = l.staging; a.pool_off = l.pool_off; a.K = l.K;
  return a;
}

int launch_snapshot_export(const SnapLaunch &l, void *stream) {
  hipLaunchKernelGGL(ctc_stream_export_kernel, dim3((unsigned)l.B), dim3(kSnapThreads), 0, (hipStream_t)stream, snap_args(l));
  return (int)hipGetLastError();
}

int launch_snapshot_import(const SnapLaunch &l, void *stream) {
  hipLaunchKernelGGL(ctc_stream_import_kernel, dim3((unsigned)l.B), dim3(kSnapThreads), 0, (hipStream_t)stream, snap_args(l));
  return (int)hipGetLastError();
}

}  // namespace ctcsnap
