// blank_skip.hip -- the blank-frame filter of blank_skip.h on the device, and its C ABI (include/ctcdecode_amd.h "Blank-frame
// filter").  A translation unit of its own: it runs in front of the pre-passes and behind the decode, and no kernel of
// ctcdecode_amd.hip or decode_kernels.hip sees it.
//   ctc_blank_scan_kernel<DT>     one workgroup per utterance: the kept frames' indices in order, their count, a zero tail
//   ctc_blank_gather_kernel<W>    one workgroup per (utterance, tile of kept frames): the kept rows, densely, into the call's private copy
//   ctc_remap_timesteps_kernel    padded results: timesteps[b][p][i] = kept[b][timesteps[b][p][i]] over the valid prefixes
//   ctc_remap_compact_kernel      compact results: the same on the upper 16 bits of every label record an item's entries own
#include <hip/hip_runtime.h>

#include <string>
#include <thread>
#include <vector>

#include "../../include/ctcdecode_amd.h"
#include "blank_skip.h"
#include "device_guard.h"

namespace ctcskip {

// Scan.  Chunks of kScanThreads frames, one strided blank value per thread; a kept frame's rank = the carry of the chunks before it
// + the kept frames of the waves before its own (LDS) + those of the lanes before its own (ballot, mbcnt).
template <int DT>
__global__ void __launch_bounds__(kScanThreads) ctc_blank_scan_kernel(const void *rows, const int32_t *seq_lens, int T, int V, int blank_id, float c,
                                                                      int32_t *kept, int32_t *kept_lens) {
  __shared__ int s_wave[2][kScanWaves];  // (two sets: a chunk's counts are read while the next chunk's are written)
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6;
  const int n = clamped_len(seq_lens, b, T);
  int32_t *kb = kept + (size_t)b * T;
  int carry = 0, set = 0;
  for (int t0 = 0; t0 < n; t0 += kScanThreads, set ^= 1) {
    const int t = t0 + tid;
    const bool keep = t < n && frame_kept<DT>(rows, b, t, T, V, blank_id, c);
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
    if (keep) kb[carry + below + before] = t;  // (a rank below the number of frames looked at so far: < n <= T)
    carry += total;
  }
  if (tid == 0) kept_lens[b] = carry;
  for (int i = carry + tid; i < T; i += kScanThreads) kb[i] = 0;
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Gather.  The tile's kept rows are consecutive in the output; W = the copy's word: 16 bytes when rows are whole 16-byte words on
// both sides, else the element (2 or 4 bytes: rows of an odd number of elements are only element-aligned).
template <typename W>
__global__ void __launch_bounds__(kGatherThreads) ctc_blank_gather_kernel(const W *in, W *out, const int32_t *kept, const int32_t *kept_lens, int T,
                                                                          unsigned row_words, int tile_rows, unsigned tiles) {
  const int b = (int)(blockIdx.x / tiles);
  gather_tile<W>(in, out, kept, kept_lens, b, (int)(blockIdx.x - (unsigned)b * tiles), T, row_words, tile_rows, threadIdx.x, (unsigned)kGatherThreads,
                 [](W *d, const W &v) { __builtin_nontemporal_store(v, d); });
}

__global__ void __launch_bounds__(kRemapThreads) ctc_remap_timesteps_kernel(int32_t *timesteps, const int32_t *out_lens, const int32_t *kept,
                                                                            const int32_t *kept_lens, long long n_rows, int K, int T) {
  const long long row = (long long)blockIdx.x * (kRemapThreads / 64) + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const int b = (int)(row / K);
  const int nk = clamp_count(kept_lens[b], T), L = clamp_count(out_lens[row], T);
  const int32_t *kb = kept + (size_t)b * T;
  int32_t *ts = timesteps + (size_t)row * T;
  for (int i = (int)(threadIdx.x & 63); i < L; i += 64) {
    const int32_t s = ts[i], m = remap_step(s, kb, nk);
    if (m != s) ts[i] = m;
  }
}

// (the record layout: expand_compact_kernel of ctcdecode_amd.hip; entry j owns labels [off, off + length - shared), inside the
//  item's [first, first + total) of c_hdr)
__global__ void __launch_bounds__(kRemapThreads) ctc_remap_compact_kernel(const int32_t *hdr, const int32_t *ent, uint32_t *labels, const int32_t *kept,
                                                                          const int32_t *kept_lens, int K, int T) {
  const int b = (int)blockIdx.x;
  const int nk = clamp_count(kept_lens[b], T);
  const int nres = clamp_count(hdr[(size_t)b * 4], K);
  const uint32_t total = (uint32_t)hdr[(size_t)b * 4 + 1], first = (uint32_t)hdr[(size_t)b * 4 + 2];
  const int32_t *kb = kept + (size_t)b * T;
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  for (int j = wave; j < nres; j += kRemapThreads / 64) {
    const int4 e = *reinterpret_cast<const int4 *>(ent + ((size_t)b * K + j) * 4);
    const int own = e.z - (j == 0 ? 0 : e.y);
    for (int q = lane; q < own; q += 64) {
      const uint32_t at = (uint32_t)e.w + (uint32_t)q;
      if (at - first >= total) continue;  // (outside the item's own labels: not this call's to touch)
      const uint32_t rec = labels[at], m = remap_record(rec, kb, nk);
      if (m != rec) labels[at] = m;
    }
  }
}

namespace {

int hip_fail(const char *what, hipError_t e) { return skip_fail(CTCD_EHIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str()); }

template <typename W>
hipError_t launch_gather(const void *in, void *out, const int32_t *kept, const int32_t *kept_lens, int B, int T, size_t row_bytes, hipStream_t s) {
  const int tile_rows = gather_tile_rows(row_bytes), tiles = gather_tiles(T, tile_rows);
  if ((long long)tiles * B > 0x7fffffffLL) return hipErrorInvalidConfiguration;
  hipLaunchKernelGGL(ctc_blank_gather_kernel<W>, dim3((unsigned)tiles * (unsigned)B), dim3(kGatherThreads), 0, s, (const W *)in, (W *)out, kept, kept_lens, T,
                     (unsigned)(row_bytes / sizeof(W)), tile_rows, (unsigned)tiles);
  return hipGetLastError();
}

}  // namespace

// the gather on its own, for the filter of live streams (stream_blank_skip.h): `kept` / `kept_lens` are a chunk scan's
int launch_blank_gather(const void *in, void *out, const int32_t *kept, const int32_t *kept_lens, int B, int T, int V, int dtype, void *stream) {
  const size_t eb = elem_bytes(dtype), row_bytes = (size_t)V * eb;
  hipStream_t s = (hipStream_t)stream;
  if (gather_vec16(row_bytes, (uintptr_t)in, (uintptr_t)out)) return (int)launch_gather<u32x4>(in, out, kept, kept_lens, B, T, row_bytes, s);
  if (eb == 4) return (int)launch_gather<uint32_t>(in, out, kept, kept_lens, B, T, row_bytes, s);
  return (int)launch_gather<uint16_t>(in, out, kept, kept_lens, B, T, row_bytes, s);
}
}  // namespace ctcskip

using namespace ctcskip;

extern "C" {

int ctcd_blank_skip(ctcd_decoder *d, const void *x, const int32_t *seq_lens, int B, int T, int V, int blank_id, float cmp, void *out_rows,
                    int32_t *out_lens, int32_t *out_kept, void *stream) {
  if (!d || !x || !out_rows || !out_lens || !out_kept) return skip_fail(CTCD_EINVAL, "ctcd_blank_skip: null argument");
  if (B <= 0 || T <= 0 || V <= 0) return skip_fail(CTCD_EINVAL, "ctcd_blank_skip: B, T, V > 0 required");
  if (blank_id < 0 || blank_id >= V) return skip_fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (x == out_rows) return skip_fail(CTCD_EINVAL, "ctcd_blank_skip: the filter is not in place");
  SkipDecoderInfo inf;
  if (const int rc = skip_decoder_info(d, &inf)) return rc;
  ctcdev::DeviceGuard guard(inf.device);
  if (guard.err != hipSuccess) return hip_fail("hipSetDevice", guard.err);
  hipStream_t s = (hipStream_t)stream;
  switch (inf.in_dtype) {
    case CTCD_DTYPE_F16:
      hipLaunchKernelGGL(ctc_blank_scan_kernel<kSkipF16>, dim3((unsigned)B), dim3(kScanThreads), 0, s, x, seq_lens, T, V, blank_id, cmp, out_kept, out_lens);
      break;
    case CTCD_DTYPE_BF16:
      hipLaunchKernelGGL(ctc_blank_scan_kernel<kSkipBF16>, dim3((unsigned)B), dim3(kScanThreads), 0, s, x, seq_lens, T, V, blank_id, cmp, out_kept, out_lens);
      break;
    default:
      hipLaunchKernelGGL(ctc_blank_scan_kernel<kSkipF32>, dim3((unsigned)B), dim3(kScanThreads), 0, s, x, seq_lens, T, V, blank_id, cmp, out_kept, out_lens);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("blank scan", e);
  const size_t eb = elem_bytes(inf.in_dtype), row_bytes = (size_t)V * eb;
  if (gather_vec16(row_bytes, (uintptr_t)x, (uintptr_t)out_rows)) e = launch_gather<u32x4>(x, out_rows, out_kept, out_lens, B, T, row_bytes, s);
  else if (eb == 4) e = launch_gather<uint32_t>(x, out_rows, out_kept, out_lens, B, T, row_bytes, s);
  else e = launch_gather<uint16_t>(x, out_rows, out_kept, out_lens, B, T, row_bytes, s);
  if (e != hipSuccess) return hip_fail("blank gather", e);
  return CTCD_OK;
}

int ctcd_remap_timesteps(ctcd_decoder *d, int32_t *timesteps, const int32_t *out_lens, const int32_t *kept, const int32_t *kept_lens, int B, int K, int T,
                         void *stream) {
  if (!d || !timesteps || !out_lens || !kept || !kept_lens) return skip_fail(CTCD_EINVAL, "ctcd_remap_timesteps: null argument");
  if (B <= 0 || K <= 0 || T <= 0) return skip_fail(CTCD_EINVAL, "ctcd_remap_timesteps: B, K, T > 0 required");
  SkipDecoderInfo inf;
  if (const int rc = skip_decoder_info(d, &inf)) return rc;
  ctcdev::DeviceGuard guard(inf.device);
  if (guard.err != hipSuccess) return hip_fail("hipSetDevice", guard.err);
  const long long n_rows = (long long)B * K, per = kRemapThreads / 64;
  if ((n_rows + per - 1) / per > 0x7fffffffLL) return skip_fail(CTCD_EUNSUPPORTED, "ctcd_remap_timesteps: too many result rows for one launch");
  hipLaunchKernelGGL(ctc_remap_timesteps_kernel, dim3((unsigned)((n_rows + per - 1) / per)), dim3(kRemapThreads), 0, (hipStream_t)stream, timesteps, out_lens,
                     kept, kept_lens, n_rows, K, T);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CTCD_OK : hip_fail("remap of the padded results", e);
}

int ctcd_remap_compact(ctcd_decoder *d, const int32_t *c_hdr, const int32_t *c_ent, uint32_t *c_labels, const int32_t *kept, const int32_t *kept_lens, int B,
                       int K, int T, void *stream) {
  if (!d || !c_hdr || !c_ent || !c_labels || !kept || !kept_lens) return skip_fail(CTCD_EINVAL, "ctcd_remap_compact: null argument");
  if (B <= 0 || K <= 0 || T <= 0) return skip_fail(CTCD_EINVAL, "ctcd_remap_compact: B, K, T > 0 required");
  if (T > 65536) return skip_fail(CTCD_EINVAL, "ctcd_remap_compact: compact results hold frame numbers below 65536");
  SkipDecoderInfo inf;
  if (const int rc = skip_decoder_info(d, &inf)) return rc;
  ctcdev::DeviceGuard guard(inf.device);
  if (guard.err != hipSuccess) return hip_fail("hipSetDevice", guard.err);
  hipLaunchKernelGGL(ctc_remap_compact_kernel, dim3((unsigned)B), dim3(kRemapThreads), 0, (hipStream_t)stream, c_hdr, c_ent, c_labels, kept, kept_lens, K, T);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CTCD_OK : hip_fail("remap of the compact results", e);
}

int ctcd_remap_timesteps_host(int32_t *timesteps, const int32_t *out_lens, const int32_t *kept, const int32_t *kept_lens, int B, int K, int T,
                              int num_threads) {
  if (!timesteps || !out_lens || !kept || !kept_lens) return skip_fail(CTCD_EINVAL, "ctcd_remap_timesteps_host: null argument");
  if (B <= 0 || K <= 0 || T <= 0) return skip_fail(CTCD_EINVAL, "ctcd_remap_timesteps_host: B, K, T > 0 required");
  int todo = 0;  // utterances that lost frames (remap_timesteps_item_host leaves the others alone): no thread is started for nothing
  for (int b = 0; b < B; ++b) {
    const int nk = clamp_count(kept_lens[b], T);
    todo += nk > 0 && kept[(size_t)b * T + nk - 1] != nk - 1;
  }
  if (todo == 0) return CTCD_OK;
  const int cap = num_threads > 64 ? 64 : num_threads;
  const int nth = cap < 1 ? 1 : (cap > todo ? todo : cap);
  auto part = [=](int k) {  // items k, k + nth, ...: the valid prefixes alone are read and written
    for (int b = k; b < B; b += nth) remap_timesteps_item_host(timesteps, out_lens, kept, kept_lens, b, K, T);
  };
  std::vector<std::thread> th;
  for (int k = 1; k < nth; ++k) th.emplace_back(part, k);
  part(0);
  for (auto &t : th) t.join();
  return CTCD_OK;
}

}  // extern "C"
