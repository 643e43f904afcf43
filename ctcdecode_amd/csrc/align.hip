// align.hip -- CTC forced alignment of align.h on the device, and its C ABI (include/ctcdecode_amd.h "Forced alignment").  A
// translation unit of its own: it runs behind a decode on tensors that decode left in HBM, and no kernel of ctcdecode_amd.hip or
// decode_kernels.hip sees it.
//   ctc_align_kernel<DT, PROB, CLS>   persistent workgroups of four waves, each with its own slot of the decoder's scratch for the
//                                     back-pointers.  Hypotheses are classed in groups of four consecutive rows: a group whose rows
//                                     all fit a wave (S <= 64) runs them side by side, one per wave, without a barrier (CLS 0:
//                                     workgroup g takes the groups g, g + grid, ...); the rows of any other group run on a whole
//                                     workgroup each, 1, 4 or 16 states per lane (CLS: workgroup g takes the rows g, g + grid, ...),
//                                     one barrier per frame.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "align.h"

namespace ctcalign {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// words [0, count) at p <- 0 by the unit's threads: single words up to the first 16-byte boundary, 16-byte stores, single words
__device__ __forceinline__ void zero_words(int32_t *p, int count, int utid, int nt) {
  if (count <= 0) return;
  int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
  if (head > count) head = count;
  const int body = (count - head) >> 2, tail0 = head + body * 4;
  if (utid < head) p[utid] = 0;
  i32x4 z;
  z.x = 0; z.y = 0; z.z = 0; z.w = 0;
  i32x4 *q = reinterpret_cast<i32x4 *>(p + head);
  for (int i = utid; i < body; i += nt) q[i] = z;
  if (utid < count - tail0) p[tail0 + utid] = 0;
}

// a frame's back-pointers of NPL states per lane, whole words: the lanes that share a word OR their bits together
template <int NPL> __device__ __forceinline__ uint32_t pack_word(uint32_t bits, int lane) {
  if (NPL == 16) return bits;
  constexpr int kLanes = 16 / NPL;  // lanes per word: 16 (NPL 1) or 4 (NPL 4)
  uint32_t w = bits << (2u * NPL * (unsigned)(lane & (kLanes - 1)));
#pragma unroll
  for (int m = 1; m < kLanes; m <<= 1) w |= (uint32_t)__shfl_xor((int)w, m, 64);
  return w;
}

// One hypothesis on one unit: WAVES = 1 (a wave, utid = its lane) or kAlignWaves (the workgroup, utid = the thread), NPL states per
// lane -- lane u holds states u * NPL .. u * NPL + NPL - 1 in registers, so that the neighbours s - 1 and s - 2 of all but a lane's
// first two states are its own.  The others come from the lane before it (__shfl_up) and, at a wave's first lane, from the wave before
// it through `xch` (two floats per wave and frame parity, written behind each frame, one barrier per frame).  The row was validated
// by the caller: 0 <= L <= n, S = 2L + 1 <= 64 * WAVES * NPL, every label in [0, V) and no blank.
template <int WAVES, int NPL, int DT, bool PROB>
__device__ __forceinline__ void align_row(const void *probs, size_t row0, int n, int V, int blank, const int32_t *tok, int L, uint32_t *bp, float *xch,
                                          float *fin, int32_t *st, int32_t *en, float *score, int L_stride, int utid) {
  constexpr int NT = 64 * WAVES;
  constexpr int CH = NPL == 1 ? 8 : (NPL == 4 ? 4 : 2);  // frames whose log-probabilities are in flight while a chunk is computed
  const int lane = utid & 63, wave = utid >> 6;
  const int S = n_states(L), wpf = bp_row_words(S), s0 = utid * NPL;
  // the lane's states: the column each gathers, and which of them have the third predecessor (frame-invariant).  States at or beyond
  // S gather the blank's column and compute on: no state below them ever reads them, and the back-trace starts below them.
  constexpr unsigned kElem = DT == ctcskip::kSkipF32 ? 4u : 2u;
  unsigned zo[NPL];  // (byte offsets inside a frame's row, 32 bits: a frame's address is its uniform base plus these)
  unsigned has2 = 0u;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int s = s0 + k;
    zo[k] = (unsigned)blank * kElem;
    if (s < S) {
      if (s & 1) zo[k] = (unsigned)tok[s >> 1] * kElem;
      if (state_skips(tok, s)) has2 |= 1u << k;
    }
  }
  auto load = [&](float(&dst)[NPL], int t) {  // frame t's values as they lie in memory (a frame at or beyond n: frame n - 1's, unused)
    const char *fr = (const char *)probs + (row0 + (size_t)(t < n ? t : n - 1)) * (size_t)V * kElem;
#pragma unroll
    for (int k = 0; k < NPL; ++k) dst[k] = ctcskip::widen_at<DT>(fr + (size_t)zo[k], 0);
  };
  auto convert = [&](float(&v)[NPL]) {
    if (PROB) {
#pragma unroll
      for (int k = 0; k < NPL; ++k) v[k] = prob_to_lp(v[k]);
    }
  };
  // this frame's last two states of the wave, for the wave behind it
  float d[NPL];
  auto publish = [&](int par) {
    if (WAVES > 1) {
      const float before = NPL >= 2 ? d[NPL >= 2 ? NPL - 2 : 0] : __shfl_up(d[0], 1, 64);
      if (lane == 63) {
        xch[(par * WAVES + wave) * 2] = d[NPL - 1];
        xch[(par * WAVES + wave) * 2 + 1] = before;
      }
      __syncthreads();
    }
  };

  float cur[CH][NPL], nxt[CH][NPL];
  load(cur[0], 0);
  convert(cur[0]);
#pragma unroll
  for (int k = 0; k < NPL; ++k) d[k] = (s0 + k < 2 && s0 + k < S) ? cur[0][k] : neg_inf();
  publish(0);
#pragma unroll
  for (int c = 0; c < CH; ++c) load(cur[c], 1 + c);
#pragma unroll
  for (int c = 0; c < CH; ++c) convert(cur[c]);
  for (int t0 = 1; t0 < n; t0 += CH) {
#pragma unroll
    for (int c = 0; c < CH; ++c) load(nxt[c], t0 + CH + c);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int t = t0 + c;
      if (t < n) {  // (the same for every lane of the unit)
        // states s0 - 1 and s0 - 2 of frame t - 1
        float a_in, b_in;
        if (NPL == 1) {
          a_in = __shfl_up(d[0], 1, 64);
          b_in = __shfl_up(d[0], 2, 64);
        } else {
          a_in = __shfl_up(d[NPL - 1], 1, 64);
          b_in = __shfl_up(d[NPL >= 2 ? NPL - 2 : 0], 1, 64);
        }
        if (WAVES > 1 && wave > 0) {
          const int at = (((t - 1) & 1) * WAVES + wave - 1) * 2;
          if (lane == 0) {
            a_in = xch[at];
            b_in = xch[at + 1];
          }
          if (NPL == 1 && lane == 1) b_in = xch[at];
        }
        if (utid == 0) a_in = neg_inf();  // (state 0 has no predecessor but itself: -inf never exceeds what it is compared with)
        uint32_t bits = 0u;
#pragma unroll
        for (int k = NPL - 1; k >= 0; --k) {  // (descending: d[k - 1] and d[k - 2] are still frame t - 1's)
          const float p1 = k >= 1 ? d[k >= 1 ? k - 1 : 0] : a_in;
          const float p2 = k >= 2 ? d[k >= 2 ? k - 2 : 0] : (k == 1 ? a_in : b_in);
          const Cell cell = cell_update(cur[c][k], d[k], p1, true, p2, (has2 >> k) & 1u);
          d[k] = cell.v;
          bits |= cell.bp << (2 * k);
        }
        const uint32_t word = pack_word<NPL>(bits, lane);
        const int widx = s0 >> 4;
        if ((s0 & 15) == 0 && widx < wpf) bp[(size_t)t * wpf + widx] = word;
        publish(t & 1);
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
      for (int k = 0; k < NPL; ++k) cur[c][k] = nxt[c][k];
      convert(cur[c]);
    }
  }
  // the end state: d[n-1][S-1] and d[n-1][S-2], from the lanes that hold them
  float mine1 = 0.0f, mine2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    if (s0 + k == S - 1) mine1 = d[k];
    if (s0 + k == S - 2) mine2 = d[k];
  }
  __threadfence();  // (the back-pointer rows are read back below, by the unit's first wave)
  float d_last, d_before = 0.0f;
  if (WAVES > 1) {
    if (s0 <= S - 1 && S - 1 < s0 + NPL) fin[0] = mine1;
    if (s0 <= S - 2 && S - 2 < s0 + NPL) fin[1] = mine2;
    __syncthreads();
    d_last = fin[0];
    if (L >= 1) d_before = fin[1];
  } else {
    d_last = __shfl(mine1, (S - 1) / NPL, 64);
    if (L >= 1) d_before = __shfl(mine2, (S - 2) / NPL, 64);
  }
  const int e = end_state(L, d_last, d_before);
  const float sc = e == S - 1 ? d_last : d_before;
  const bool aligned = sc > neg_inf();
  if (utid == 0) *score = sc;
  if (aligned && L > 0 && wave == 0) {
    // The back-trace, on one wave.  Sixteen frames at a time: over them the path's state stays within 30 states of where it is, i.e.
    // within three words of a row, so the 48 words the chunk can need are loaded by 48 lanes at once and the sixteen dependent steps
    // pick theirs by shuffle.  Every lane follows the path; lane 0 writes the spans.
    const bool wr = lane == 0;
    trace_begin(e, n, en, wr);
    int s = e;
    for (int t = n - 1; t >= 1; t -= 16) {
      const int w_lo = (s >> 4) - 2, j = lane / 3, w = w_lo + lane % 3, tt = t - j;
      uint32_t val = 0u;
      if (lane < 48 && tt >= 1 && w >= 0 && w < wpf) val = __hip_atomic_load(bp + (size_t)tt * wpf + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (t - q >= 1) {
          const uint32_t word = (uint32_t)__shfl((int)val, q * 3 + ((s >> 4) - w_lo), 64);
          s = trace_step(s, bp_get(word, s), t - q, st, en, wr);
        }
      }
    }
    trace_end(s, st, wr);
  }
  // positions at or beyond the row's length -- every position of a row that is not aligned -- are 0
  const int from = aligned ? L : 0;
  zero_words(st + from, L_stride - from, utid, NT);
  zero_words(en + from, L_stride - from, utid, NT);
}

// a row that runs no recurrence: the outputs zero, the score given
template <int WAVES> __device__ __forceinline__ void blank_row(int32_t *st, int32_t *en, float *score, float sc, int L_stride, int utid) {
  zero_words(st, L_stride, utid, 64 * WAVES);
  zero_words(en, L_stride, utid, 64 * WAVES);
  if (utid == 0) *score = sc;
}

// what a wave found out about its row of the group
enum : int { kRowNone = -1, kRowInvalid = -2, kRowNoPath = -3 };  // else: L, a valid row that runs the recurrence (0 <= L <= n, n >= 1)

// The rows fall into four classes, and each class has a kernel of its own (CLS), so that each gets the registers its class needs and
// no more: 0 = the rows of a group of four that all fit a wave (S <= 64, and the rows that run no recurrence), one per wave side by
// side; 1 / 4 / 16 = the rows of every other group, on the whole workgroup with that many states per lane (rows of such a group that
// run no recurrence: class 1).  Every kernel walks all rows and classes their groups alike; a row is written by exactly one of them.
template <int DT, bool PROB, int CLS>
__global__ void __launch_bounds__(kAlignThreads) ctc_align_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens,
                                                                  const int32_t *lens, int R, int L_stride, long long rows, char *scratch, size_t slot_bytes,
                                                                  int32_t *out_st, int32_t *out_en, float *out_sc, int32_t *status) {
  __shared__ float s_xch[2 * kAlignWaves * 2];
  __shared__ float s_fin[2];
  __shared__ int s_row[kAlignWaves];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t *slot = reinterpret_cast<uint32_t *>(scratch + (size_t)blockIdx.x * slot_bytes);
  // the unit a workgroup takes at a time: a group of four rows side by side (CLS 0), or one row (it still looks at the row's whole
  // group, to class it as the kernel of class 0 does)
  const long long units = CLS == 0 ? align_groups(rows) : rows;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    const long long g = CLS == 0 ? u : u / kAlignWaves;
    // wave w looks at row 4g + w: its length against L_stride, then its labels against the vocabulary
    const long long h = g * kAlignWaves + wave;
    int what = kRowNone;
    if (h < rows) {
      const int b = (int)(h / R), len = lens[h];
      bool ok = len_ok(len, L_stride);
      if (ok) {
        const int32_t *y = tokens + (size_t)h * L_stride;
        bool bad = false;
        for (int i = lane; i < len; i += 64) bad |= !label_ok(y[i], V, blank);
        ok = __ballot(bad) == 0ull;
      }
      const int n = ctcskip::clamped_len(seq_lens, b, T);
      what = !ok ? kRowInvalid : ((n == 0 || len > n) ? kRowNoPath : len);
      if (!ok && status && lane == 0) status[b] = ALIGN_BAD_ROW;  // (raised only)
    }
    if (lane == 0) s_row[wave] = what;
    __syncthreads();
    bool all_short = true;
#pragma unroll
    for (int w = 0; w < kAlignWaves; ++w) all_short = all_short && n_states(s_row[w]) <= 64;  // (the negative codes count as short)
    if (CLS == 0) {
      if (all_short && h < rows) {
        const int b = (int)(h / R), n = ctcskip::clamped_len(seq_lens, b, T);
        int32_t *st = out_st + (size_t)h * L_stride, *en = out_en + (size_t)h * L_stride;
        if (what < 0)
          blank_row<1>(st, en, out_sc + h, what == kRowInvalid || (n == 0 && lens[h] == 0) ? 0.0f : neg_inf(), L_stride, lane);
        else
          align_row<1, 1, DT, PROB>(probs, (size_t)b * T, n, V, blank, tokens + (size_t)h * L_stride, what, slot + (size_t)wave * align_wave_words(T), s_xch,
                                    s_fin, st, en, out_sc + h, L_stride, lane);
      }
    } else if (!all_short) {
      const int code = s_row[(int)(u % kAlignWaves)];
      const int b = (int)(u / R), n = ctcskip::clamped_len(seq_lens, b, T);
      int32_t *st = out_st + (size_t)u * L_stride, *en = out_en + (size_t)u * L_stride;
      if (code < 0) {
        if (CLS == 1) blank_row<kAlignWaves>(st, en, out_sc + u, code == kRowInvalid || (n == 0 && lens[u] == 0) ? 0.0f : neg_inf(), L_stride, tid);
      } else if (align_npl(n_states(code)) == CLS) {  // (the launcher refuses shapes whose rows can exceed kAlignMaxStates)
        align_row<kAlignWaves, CLS == 0 ? 1 : CLS, DT, PROB>(probs, (size_t)b * T, n, V, blank, tokens + (size_t)u * L_stride, code, slot, s_xch, s_fin, st, en,
                                                             out_sc + u, L_stride, tid);
      }
    }
    __syncthreads();  // (s_row, s_xch, s_fin and the slot belong to the next unit)
  }
}

namespace {
struct AlignDeviceGuard {  // the caller's current device is put back on exit (as every entry point of ctcdecode_amd.hip does)
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit AlignDeviceGuard(int dev) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != dev) prev = cur;
    if (cur != dev) err = hipSetDevice(dev);
  }
  ~AlignDeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// the kernels of the classes the shape allows (S <= 2 * min(L_stride, T) + 1), one behind the other on the stream
template <int DT, bool PROB>
hipError_t launch(unsigned row_grid, hipStream_t s, const void *probs, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens, const int32_t *lens, int R,
                  int L_stride, long long rows, char *scratch, size_t slot_bytes, int32_t *st, int32_t *en, float *sc, int32_t *status) {
  const int smax = n_states(align_lmax(T, L_stride));
#define CTC_ALIGN_CLASS(CLS)                                                                                                                              \
  hipLaunchKernelGGL((ctc_align_kernel<DT, PROB, CLS>), dim3(grid), dim3(kAlignThreads), 0, s, probs, seq_lens, T, V, blank, tokens, lens, R, L_stride, rows, \
                     scratch, slot_bytes, st, en, sc, status)
  // class 0 takes a group of four rows per workgroup at a time, the other classes one row
  const long long groups = align_groups(rows);
  unsigned grid = (long long)row_grid > groups ? (unsigned)groups : row_grid;
  CTC_ALIGN_CLASS(0);
  grid = row_grid;
  if (smax > 64) CTC_ALIGN_CLASS(1);
  if (smax > kAlignThreads) CTC_ALIGN_CLASS(4);
  if (smax > kAlignThreads * 4) CTC_ALIGN_CLASS(16);
#undef CTC_ALIGN_CLASS
  return hipGetLastError();
}
}  // namespace
}  // namespace ctcalign

using namespace ctcalign;

extern "C" {

int ctcd_ctc_align(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *tokens,
                   const int32_t *lens, int R, int L_stride, int32_t *out_start, int32_t *out_end, float *out_scores, int32_t *status, void *stream) {
  if (!d) return align_fail(CTCD_EINVAL, "decoder == NULL");
  if (B < 0 || T < 0 || V < 1 || R < 0 || L_stride < 0) return align_fail(CTCD_EINVAL, "ctcd_ctc_align: B, T, R, L_stride >= 0 and V >= 1 required");
  if (blank_id < 0 || blank_id >= V) return align_fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (log_input < 0 || log_input > 2) return align_fail(CTCD_EINVAL, "ctcd_ctc_align: log_input must be 0, 1 or 2");
  const long long rows = (long long)B * R;
  if (rows == 0) return CTCD_OK;
  if (!tokens && L_stride > 0) return align_fail(CTCD_EINVAL, "ctcd_ctc_align: null tensor");
  if (!lens || !out_scores || (L_stride > 0 && (!out_start || !out_end)) || (T > 0 && !probs)) return align_fail(CTCD_EINVAL, "ctcd_ctc_align: null tensor");
  if (align_lmax(T, L_stride) > kAlignMaxLabels)
    return align_fail(CTCD_EUNSUPPORTED, "ctcd_ctc_align: rows of more than 2047 labels (min(L_stride, T) > 2047) are not built");
  if (V > (1 << 28)) return align_fail(CTCD_EUNSUPPORTED, "ctcd_ctc_align: V > 2^28");  // (a row's byte offsets are 32 bits)
  if (rows > 0x7fffffffLL) return align_fail(CTCD_EUNSUPPORTED, "ctcd_ctc_align: too many rows for one launch");
  AlignDecoderInfo inf;
  if (const int rc = align_decoder_info(d, &inf)) return rc;
  AlignDeviceGuard guard(inf.device);
  if (guard.err != hipSuccess) return align_fail(CTCD_EHIP, (std::string("hipSetDevice: ") + hipGetErrorString(guard.err)).c_str());
  int dt = inf.in_dtype;
  if (log_input == 2 && T > 0) {  // raw logits: the log-softmax pass into the decoder's float32 rows, then log-probabilities
    const float *rows32 = nullptr;
    if (const int rc = align_lsm_rows(d, probs, seq_lens, B, T, V, stream, &rows32)) return rc;
    probs = rows32;
    dt = CTCD_DTYPE_F32;
  }
  const size_t slot = align_slot_bytes(T, L_stride);
  const long long grid = align_grid(rows, inf.budget, slot);
  void *scratch = nullptr;
  if (const int rc = align_scratch(d, (size_t)grid * slot, &scratch)) return rc;
  align_note_grid(d, grid);
  hipStream_t s = (hipStream_t)stream;
  const bool prob = log_input == 0;
  hipError_t e;
#define CTC_ALIGN_LAUNCH(DT, PROB) \
  launch<DT, PROB>((unsigned)grid, s, probs, seq_lens, T, V, blank_id, tokens, lens, R, L_stride, rows, (char *)scratch, slot, out_start, out_end, out_scores, status)
  if (dt == CTCD_DTYPE_F16) e = prob ? CTC_ALIGN_LAUNCH(ctcskip::kSkipF16, true) : CTC_ALIGN_LAUNCH(ctcskip::kSkipF16, false);
  else if (dt == CTCD_DTYPE_BF16) e = prob ? CTC_ALIGN_LAUNCH(ctcskip::kSkipBF16, true) : CTC_ALIGN_LAUNCH(ctcskip::kSkipBF16, false);
  else e = prob ? CTC_ALIGN_LAUNCH(ctcskip::kSkipF32, true) : CTC_ALIGN_LAUNCH(ctcskip::kSkipF32, false);
#undef CTC_ALIGN_LAUNCH
  return e == hipSuccess ? CTCD_OK : align_fail(CTCD_EHIP, (std::string("alignment: ") + hipGetErrorString(e)).c_str());
}

}  // extern "C"
