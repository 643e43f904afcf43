// stream_blank_skip.hip -- the blank-frame filter of live streams on the device (stream_blank_skip.h).  A translation unit of its
// own: its kernels run in front of a chunk's pre-passes and behind whatever a streaming call reports, and no kernel of
// ctcdecode_amd.hip, decode_kernels.hip or blank_skip.hip sees them (the gather between scan and decode is blank_skip.hip's).
//   ctc_stream_scan_kernel<DT>         one workgroup per stream: the chunk's kept frames in order, their count, the stream's map continued
//   ctc_stream_remap_rows_kernel       result rows of any stride: ts = map_b[ts] over the reported part of every row (one wave per row)
//   ctc_stream_remap_compact_kernel    the same on the frame half of every label record an item's entries own (one workgroup per item)
#include <hip/hip_runtime.h>

#include "../../include/ctcdecode_amd.h"
#include "stream_blank_skip.h"

namespace ctcsskip {

// Scan with carry.  blank_skip.hip's scan: passes of kScanThreads frames, one strided blank value per thread; a kept frame's rank in
// the chunk = the carry of the passes before it + the kept frames of the waves before its own (LDS) + those of the lanes before its
// own (ballot, mbcnt).  The stream's bases come from the call's argument table.
template <int DT>
__global__ void __launch_bounds__(kScanThreads) ctc_stream_scan_kernel(const void *rows, const int32_t *seq_lens, const StreamSkipItem *tab, int T, int V,
                                                                       int blank_id, float c, int32_t *kept, int32_t *kept_lens) {
  __shared__ int s_wave[2][kScanWaves];  // (two sets: a pass's counts are read while the next pass's are written)
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6;
  const int n = ctcskip::clamped_len(seq_lens, b, T);
  const StreamSkipItem it = tab[b];
  int32_t *kb = kept + (size_t)b * T;
  int carry = 0, set = 0;
  for (int t0 = 0; t0 < n; t0 += kScanThreads, set ^= 1) {
    const int t = t0 + tid;
    const bool keep = t < n && ctcskip::frame_kept<DT>(rows, b, t, T, V, blank_id, c);
    const unsigned long long mask = __ballot(keep);
    const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    if ((tid & 63) == 0) s_wave[set][wave] = __popcll(mask);
    __syncthreads();
    int below = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScanWaves; ++w) {
      const int cw = s_wave[set][w];
      below += w < wave ? cw : 0;
      total += cw;
    }
    if (keep) scan_store(it, kb, chunk_rank(carry, below, before), t);  // (a rank below the frames looked at so far: < n <= T)
    carry += total;
  }
  if (tid == 0) kept_lens[b] = carry;
}

__global__ void __launch_bounds__(kRemapThreads) ctc_stream_remap_rows_kernel(int32_t *ts, const int32_t *lens, const int32_t *since,
                                                                              const StreamRemapItem *tab, long long n_rows, int rows_per_item,
                                                                              long long row_stride) {
  const long long row = (long long)blockIdx.x * (kRemapThreads / 64) + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int b = (int)(row / rows_per_item), p = (int)(row - (long long)b * rows_per_item);
  const StreamRemapItem it = tab[b];
  const int n = row_words(lens, since, row, b, row_stride);
  int32_t *r = row_base(it, ts, row, p, row_stride);
  for (int i = (int)(threadIdx.x & 63); i < n; i += 64) {
    const int32_t s = r[i], m = remap_step(s, it.map, it.frames);
    if (m != s) r[i] = m;
  }
}

// (the record layout: expand_compact_kernel of ctcdecode_amd.hip; entry j owns labels [off, off + length - shared), inside the
//  item's [first, first + total) of c_hdr)
__global__ void __launch_bounds__(kRemapThreads) ctc_stream_remap_compact_kernel(const int32_t *hdr, const int32_t *ent, uint32_t *labels,
                                                                                 const StreamRemapItem *tab, int K) {
  const int b = (int)blockIdx.x;
  const StreamRemapItem it = tab[b];
  const int nres = ctcskip::clamp_count(hdr[(size_t)b * 4], K);
  const uint32_t total = (uint32_t)hdr[(size_t)b * 4 + 1], first = (uint32_t)hdr[(size_t)b * 4 + 2];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  for (int j = wave; j < nres; j += kRemapThreads / 64) {
    const int4 e = *reinterpret_cast<const int4 *>(ent + ((size_t)b * K + j) * 4);
    const int own = e.z - (j == 0 ? 0 : e.y);
    for (int q = lane; q < own; q += 64) {
      const uint32_t at = (uint32_t)e.w + (uint32_t)q;
      if (at - first >= total) continue;  // (outside the item's own labels: not this call's to touch)
      const uint32_t rec = labels[at], m = remap_record(rec, it.map, it.frames);
      if (m != rec) labels[at] = m;
    }
  }
}

int launch_chunk_scan(const void *rows, const int32_t *seq_lens, const StreamSkipItem *tab, int B, int T, int V, int blank_id, float c, int dtype,
                      int32_t *kept, int32_t *kept_lens, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case CTCD_DTYPE_F16:
      hipLaunchKernelGGL(ctc_stream_scan_kernel<ctcskip::kSkipF16>, dim3((unsigned)B), dim3(kScanThreads), 0, s, rows, seq_lens, tab, T, V, blank_id, c, kept, kept_lens);
      break;
    case CTCD_DTYPE_BF16:
      hipLaunchKernelGGL(ctc_stream_scan_kernel<ctcskip::kSkipBF16>, dim3((unsigned)B), dim3(kScanThreads), 0, s, rows, seq_lens, tab, T, V, blank_id, c, kept, kept_lens);
      break;
    default:
      hipLaunchKernelGGL(ctc_stream_scan_kernel<ctcskip::kSkipF32>, dim3((unsigned)B), dim3(kScanThreads), 0, s, rows, seq_lens, tab, T, V, blank_id, c, kept, kept_lens);
  }
  return (int)hipGetLastError();
}

int launch_remap_rows(int32_t *ts, const int32_t *lens, const int32_t *since, const StreamRemapItem *tab, int B, int rows_per_item, long long row_stride,
                      void *stream) {
  const long long n_rows = (long long)B * rows_per_item, per = kRemapThreads / 64, blocks = (n_rows + per - 1) / per;
  if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidConfiguration;
  if (blocks == 0) return (int)hipSuccess;
  hipLaunchKernelGGL(ctc_stream_remap_rows_kernel, dim3((unsigned)blocks), dim3(kRemapThreads), 0, (hipStream_t)stream, ts, lens, since, tab, n_rows,
                     rows_per_item, row_stride);
  return (int)hipGetLastError();
}

int launch_remap_compact(const int32_t *hdr, const int32_t *ent, uint32_t *labels, const StreamRemapItem *tab, int B, int K, void *stream) {
  hipLaunchKernelGGL(ctc_stream_remap_compact_kernel, dim3((unsigned)B), dim3(kRemapThreads), 0, (hipStream_t)stream, hdr, ent, labels, tab, K);
  return (int)hipGetLastError();
}

}  // namespace ctcsskip
