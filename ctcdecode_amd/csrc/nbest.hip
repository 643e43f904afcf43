// nbest.hip -- the n-best expansion of nbest.h on the device, and its C ABI (include/ctcdecode_amd.h "n-best results").  A
// translation unit of its own: it runs behind the decode, and no kernel of ctcdecode_amd.hip or decode_kernels.hip sees it.
//   ctc_nbest_expand_kernel   one workgroup per item, one wave per selected row: compact records -> rows 0 .. n-1 of the four tensors
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "nbest.h"

namespace ctcnbest {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// inclusive prefix minimum over the wave's lanes (lane 0 first)
__device__ __forceinline__ int wave_prefix_min(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v = u < v ? u : v;
  }
  return v;
}

// One label position of a row whose segments are listed: the segment hint s is updated.  (Every index was checked when the segment
// was listed: nbest.h segment_ok / entry_view.)
__device__ __forceinline__ uint32_t row_label(const uint32_t *rag, const uint16_t *seg, const int *lcp, const int *off, int &s, int q) {
  s = seg_next(seg, lcp, s, q);
  const int o = seg[s];
  return rag[label_index((uint32_t)off[o], lcp[o], q)];
}

// The item's entry tables are staged in LDS once.  Each wave then takes selected rows p = wave, wave + #waves, ...: from the row's
// entry j it walks back over the entries 64 at a time -- a wave-wide prefix minimum over lcp names the entries that hold a piece of
// the row (nbest.h) -- lists them, and writes the row with consecutive lanes on consecutive positions (16-byte stores when VEC).
// The walk reads LDS only and ends when the pieces reach position 0; the label loads are independent of each other.
template <bool VEC>
__global__ void __launch_bounds__(kNbestMaxThreads) ctc_nbest_expand_kernel(const int32_t *hdr, const int32_t *ent, const uint32_t *rag,
                                                                            unsigned long long n_labels, const float *sc_in, const int32_t *len_in,
                                                                            int K, int T, int n, int32_t *tok, int32_t *ts, float *sc, int32_t *len,
                                                                            int32_t *status) {
  extern __shared__ int nsm[];
  int *lcp = nsm, *dep = nsm + K, *off = nsm + 2 * K, *sel = nsm + 3 * K;
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int wave = tid >> 6, lane = tid & 63, nw = nt >> 6;
  uint16_t *seg = (uint16_t *)(sel + n) + (size_t)wave * seg_stride(K);
  const ItemView it = item_view(hdr, b, K, n_labels);
  bool bad = !it.ok;
  for (int p = tid; p < n; p += nt) sel[p] = kNoEntry;
  __syncthreads();
  for (int j = tid; j < it.nres; j += nt) {
    const i32x4 w = *reinterpret_cast<const i32x4 *>(ent + ((size_t)b * K + j) * 4);
    const int32_t e4[4] = {w.x, w.y, w.z, w.w};
    const Entry e = entry_view(e4, j, K, T, it);
    lcp[j] = e.lcp; dep[j] = e.dep; off[j] = (int)e.off;
    bad |= !e.ok;
    if ((unsigned)e.row < (unsigned)n) atomicMin(&sel[e.row], j);  // (the first entry of a row in trie order, as on the host)
  }
  __syncthreads();
  // a row claimed twice: every claimant but the first reports it
  for (int j = tid; j < it.nres; j += nt) {
    const int row = ent[((size_t)b * K + j) * 4];
    if ((unsigned)row < (unsigned)n && sel[row] != j) bad = true;
  }
  for (int p = wave; p < n; p += nw) {
    const int j = sel[p];
    bool good = j != kNoEntry;
    int L = good ? dep[j] : 0, nseg = 0;
    if (L < 0) { good = false; L = 0; }
    int m = L;
    for (int base = j; good && m > 0 && base >= 0; base -= 64) {
      const int o = base - lane;
      const int l = o >= 0 ? lcp[o] : kNoEntry;
      const int incl = wave_prefix_min(l, lane);
      int before = __shfl_up(incl, 1, 64);  // the minimum over the entries nearer to j than o
      if (lane == 0 || before > m) before = m;
      const bool owns = o >= 0 && l < before;
      const bool broken = owns && !segment_ok(dep[o], before);
      const unsigned long long mask = __ballot(owns);
      if (owns) seg[nseg + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u))] = (uint16_t)o;
      nseg += __popcll(mask);  // (at most one segment per entry at or before j: nseg <= j + 1 <= K)
      const int low = __shfl(incl, 63, 64);
      m = low < m ? low : m;
      if (__ballot(broken)) good = false;
    }
    if (j != kNoEntry && !good) bad = true;
    if (!good) L = 0;
    __threadfence_block();  // the wave's own segment list is visible to all of its lanes
    int32_t *tk = tok + ((size_t)b * n + p) * T, *tt = ts + ((size_t)b * n + p) * T;
    if (VEC) {
      int s = 0;
      bool first = true;
      for (int q0 = lane * 4; q0 < T; q0 += 256) {
        int32_t c[4] = {0, 0, 0, 0}, sv[4] = {0, 0, 0, 0};
        if (q0 < L) {
          if (first) { s = seg_find(seg, lcp, nseg, q0); first = false; }
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (q0 + u < L) {
              const uint32_t v = row_label(rag, seg, lcp, off, s, q0 + u);
              c[u] = (int32_t)(v & 0xFFFFu);
              sv[u] = (int32_t)(v >> 16);
            }
        }
        i32x4 vc, vs;
        vc.x = c[0]; vc.y = c[1]; vc.z = c[2]; vc.w = c[3];
        vs.x = sv[0]; vs.y = sv[1]; vs.z = sv[2]; vs.w = sv[3];
        *reinterpret_cast<i32x4 *>(tk + q0) = vc;
        *reinterpret_cast<i32x4 *>(tt + q0) = vs;
      }
    } else {
      int s = 0;
      bool first = true;
      for (int q = lane; q < T; q += 64) {
        int32_t c = 0, sv = 0;
        if (q < L) {
          if (first) { s = seg_find(seg, lcp, nseg, q); first = false; }
          const uint32_t v = row_label(rag, seg, lcp, off, s, q);
          c = (int32_t)(v & 0xFFFFu);
          sv = (int32_t)(v >> 16);
        }
        tk[q] = c;
        tt[q] = sv;
      }
    }
    if (lane == 0) {
      if (sc) sc[(size_t)b * n + p] = good && sc_in ? sc_in[(size_t)b * K + p] : 0.0f;
      if (len) len[(size_t)b * n + p] = good ? (len_in ? len_in[(size_t)b * K + p] : L) : 0;
    }
    __threadfence_block();  // (the next row's list overwrites this one's: every lane has read it)
  }
  if (status && bad) status[b] = NBEST_BAD_RECORD;  // (raised only: a decode's own failure code stays)
}

bool nbest_expand_fits(const NbestDecoderInfo &inf, int beam, int n) {
  return beam <= kNbestMaxK && nbest_lds_bytes(beam, n, nbest_threads(n)) + 1024 <= (size_t)inf.max_lds;
}

int launch_nbest_expand(const NbestDecoderInfo &inf, const int32_t *c_hdr, const int32_t *c_ent, const uint32_t *c_labels, unsigned long long n_labels,
                        const float *sc_in, const int32_t *len_in, int B, int beam, int T, int n, int32_t *tok, int32_t *ts, float *sc, int32_t *len,
                        int32_t *status, void *stream) {
  const int threads = nbest_threads(n);
  const size_t lds = nbest_lds_bytes(beam, n, threads);
  const bool vec = nbest_vec16(T, (uintptr_t)tok, (uintptr_t)ts);
  const void *fn = vec ? (const void *)ctc_nbest_expand_kernel<true> : (const void *)ctc_nbest_expand_kernel<false>;
  hipError_t e = lds > 65536 ? hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) : hipSuccess;
  if (e == hipSuccess) {
    if (vec)
      hipLaunchKernelGGL(ctc_nbest_expand_kernel<true>, dim3((unsigned)B), dim3((unsigned)threads), lds, (hipStream_t)stream, c_hdr, c_ent, c_labels, n_labels,
                         sc_in, len_in, beam, T, n, tok, ts, sc, len, status);
    else
      hipLaunchKernelGGL(ctc_nbest_expand_kernel<false>, dim3((unsigned)B), dim3((unsigned)threads), lds, (hipStream_t)stream, c_hdr, c_ent, c_labels, n_labels,
                         sc_in, len_in, beam, T, n, tok, ts, sc, len, status);
    e = hipGetLastError();
  }
  return e == hipSuccess ? CTCD_OK : nbest_fail(CTCD_EHIP, (std::string("n-best expansion: ") + hipGetErrorString(e)).c_str());
}
}  // namespace ctcnbest

using namespace ctcnbest;

extern "C" {

int ctcd_expand_compact_nbest(ctcd_decoder *d, const int32_t *c_hdr, const int32_t *c_ent, const uint32_t *c_labels, long long n_labels, int B, int beam,
                              int T, int n_best, int32_t *out_tok, int32_t *out_ts, int32_t *status, void *stream) {
  if (!d || B < 0 || beam <= 0 || T < 0 || n_labels < 0) return nbest_fail(CTCD_EINVAL, "ctcd_expand_compact_nbest: bad arguments");
  if (n_best < 1 || n_best > beam) return nbest_fail(CTCD_EINVAL, "n_best must be an integer in [1, beam_width]");
  if (T > 65536) return nbest_fail(CTCD_EINVAL, "ctcd_expand_compact_nbest: compact results hold frame numbers below 65536");
  if (B == 0 || T == 0) return CTCD_OK;
  if (!c_hdr || !c_ent || !c_labels || !out_tok || !out_ts) return nbest_fail(CTCD_EINVAL, "ctcd_expand_compact_nbest: null tensor");
  if (beam > kNbestMaxK) return nbest_fail(CTCD_EUNSUPPORTED, "device expansion of compact results: beam_width > 4096");
  NbestDecoderInfo inf;
  if (const int rc = nbest_decoder_info(d, &inf)) return rc;
  if (!nbest_expand_fits(inf, beam, n_best))
    return nbest_fail(CTCD_EUNSUPPORTED, "device expansion of compact results: the entry tables of this beam width exceed one workgroup's LDS");
  ctcdev::DeviceGuard guard(inf.device);
  if (guard.err != hipSuccess) return nbest_fail(CTCD_EHIP, (std::string("hipSetDevice: ") + hipGetErrorString(guard.err)).c_str());
  return launch_nbest_expand(inf, c_hdr, c_ent, c_labels, (unsigned long long)n_labels, nullptr, nullptr, B, beam, T, n_best, out_tok, out_ts, nullptr, nullptr,
                             status, stream);
}

}  // extern "C"
