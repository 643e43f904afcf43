// align.hip -- CTC forced alignment of align.h on the device, and its C ABI (include/ctcdecode_amd.h "Forced alignment").  A
// translation unit of its own: it runs behind a decode on tensors that decode left in HBM, and no kernel of ctcdecode_amd.hip or
// decode_kernels.hip sees it.
//   ctc_align_kernel<DT, PROB, CLS>   persistent workgroups of four waves, each with its own slot of the decoder's scratch for the
//                                     back-pointers.  The walk over the rows, their classes (CLS) and the walk over a row's frames are
//                                     lattice_device.h's, shared with loglik.hip; here are what a cell records (its back-pointer), what
//                                     is kept of a frame (the back-pointer words) and what follows the last one (the back-trace).
// It also holds the entry prelude that ctcd_ctc_align and ctcd_ctc_loglik share (align_entry).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/ctcdecode_amd.h"
#include "align.h"
#include "device_guard.h"
#include "lattice_device.h"

namespace ctcalign {


using ctclattice::zero_words;

// a frame's back-pointers of NPL states per lane, whole words: the lanes that share a word OR their bits together
template <int NPL> __device__ __forceinline__ uint32_t pack_word(uint32_t bits, int lane) {
  if (NPL == 16) return bits;
  constexpr int kLanes = 16 / NPL;  // lanes per word: 16 (NPL 1) or 4 (NPL 4)
  uint32_t w = bits << (2u * NPL * (unsigned)(lane & (kLanes - 1)));
#pragma unroll
  for (int m = 1; m < kLanes; m <<= 1) w |= (uint32_t)__shfl_xor((int)w, m, 64);
  return w;
}

// One row's walk (lattice_device.h walk_row): the Viterbi cell, a back-pointer word per frame into the row's scratch `bp`, and behind
// the last frame the score, the back-trace into st / en and their zero tails.
template <int WAVES, int NPL> struct AlignRow {
  uint32_t *bp;
  int n, wpf;  // the item's frames; bp_row_words(S)
  int32_t *st, *en;
  float *score;
  int L_stride;
  uint32_t bits;  // the frame's back-pointers of this lane's states, so far

  __device__ __forceinline__ float cell(int k, float lp, float stay, float p1, float p2, bool has2) {
    const Cell c = cell_update(lp, stay, p1, true, p2, has2);
    bits |= c.bp << (2 * k);
    return c.v;
  }
  __device__ __forceinline__ void frame(int t, int s0, int lane) {
    const uint32_t word = pack_word<NPL>(bits, lane);
    const int widx = s0 >> 4;
    if ((s0 & 15) == 0 && widx < wpf) bp[(size_t)t * wpf + widx] = word;
    bits = 0u;
  }
  __device__ __forceinline__ void frames_done() { __threadfence(); }  // (the back-pointer rows are read back below, by the unit's first wave)
  __device__ __forceinline__ void finish(float d_last, float d_before, int L, int utid) {
    const int lane = utid & 63, wave = utid >> 6;
    const int e = end_state(L, d_last, d_before);
    const float sc = e == 2 * L ? d_last : d_before;
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
    zero_words(st + from, L_stride - from, utid, 64 * WAVES);
    zero_words(en + from, L_stride - from, utid, 64 * WAVES);
  }
};

// The rows of a launch (lattice_device.h walk_groups): where a row's labels, scratch and outputs lie.
template <int DT, bool PROB> struct AlignRows {
  const void *probs;
  int T, V, blank;
  const int32_t *tokens;
  int L_stride;
  uint32_t *slot;  // the workgroup's scratch slot
  int32_t *out_st, *out_en;
  float *out_sc;

  template <int WAVES, int NPL> __device__ __forceinline__ void run(long long row, int b, int n, int L, uint32_t *bp, int utid) {
    AlignRow<WAVES, NPL> r{bp, n, bp_row_words(n_states(L)), out_st + (size_t)row * L_stride, out_en + (size_t)row * L_stride, out_sc + row, L_stride, 0u};
    ctclattice::walk_row<WAVES, NPL, DT, PROB>(r, probs, (size_t)b * T, n, V, blank, tokens + (size_t)row * L_stride, L, utid);
  }
  __device__ __forceinline__ void short_row(long long row, int b, int n, int L, int lane, int wave) {
    run<1, 1>(row, b, n, L, slot + (size_t)wave * align_wave_words(T), lane);
  }
  template <int NPL> __device__ __forceinline__ void long_row(long long row, int b, int n, int L, int tid) { run<kAlignWaves, NPL>(row, b, n, L, slot, tid); }
  // the outputs zero, the score given
  template <int WAVES> __device__ __forceinline__ void no_row(long long row, float sc, int utid) {
    zero_words(out_st + (size_t)row * L_stride, L_stride, utid, 64 * WAVES);
    zero_words(out_en + (size_t)row * L_stride, L_stride, utid, 64 * WAVES);
    if (utid == 0) out_sc[row] = sc;
  }
};

template <int DT, bool PROB, int CLS>
__global__ void __launch_bounds__(kAlignThreads) ctc_align_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens,
                                                                  const int32_t *lens, int R, int L_stride, long long rows, char *scratch, size_t slot_bytes,
                                                                  int32_t *out_st, int32_t *out_en, float *out_sc, int32_t *status) {
  AlignRows<DT, PROB> pol{probs, T, V, blank, tokens, L_stride, reinterpret_cast<uint32_t *>(scratch + (size_t)blockIdx.x * slot_bytes), out_st, out_en, out_sc};
  ctclattice::walk_groups<CLS>(pol, seq_lens, T, V, blank, tokens, lens, R, L_stride, rows, status);
}

// What ctcd_ctc_align and ctcd_ctc_loglik do alike before their launch; `fn`: the entry point's name, for the messages.
int align_entry(const char *fn, ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *tokens,
                const int32_t *lens, int R, int L_stride, bool outputs, void *stream, ctcdev::DeviceGuard *guard, AlignEntry *e) {
  const std::string f = std::string(fn) + ": ";
  e->rows = 0;
  if (!d) return align_fail(CTCD_EINVAL, "decoder == NULL");
  if (B < 0 || T < 0 || V < 1 || R < 0 || L_stride < 0) return align_fail(CTCD_EINVAL, (f + "B, T, R, L_stride >= 0 and V >= 1 required").c_str());
  if (blank_id < 0 || blank_id >= V) return align_fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (log_input < 0 || log_input > 2) return align_fail(CTCD_EINVAL, (f + "log_input must be 0, 1 or 2").c_str());
  e->rows = (long long)B * R;
  if (e->rows == 0) return CTCD_OK;
  if ((!tokens && L_stride > 0) || !lens || !outputs || (T > 0 && !probs)) return align_fail(CTCD_EINVAL, (f + "null tensor").c_str());
  if (align_lmax(T, L_stride) > kAlignMaxLabels)
    return align_fail(CTCD_EUNSUPPORTED, (f + "rows of more than 2047 labels (min(L_stride, T) > 2047) are not built").c_str());
  if (V > (1 << 28)) return align_fail(CTCD_EUNSUPPORTED, (f + "V > 2^28").c_str());  // (a row's byte offsets are 32 bits)
  if (e->rows > 0x7fffffffLL) return align_fail(CTCD_EUNSUPPORTED, (f + "too many rows for one launch").c_str());
  if (const int rc = align_decoder_info(d, &e->inf)) return rc;
  if (guard->enter(e->inf.device) != hipSuccess) return align_fail(CTCD_EHIP, (std::string("hipSetDevice: ") + hipGetErrorString(guard->err)).c_str());
  e->probs = probs;
  e->dtype = e->inf.in_dtype;
  if (log_input == 2 && T > 0) {  // raw logits: the log-softmax pass into the decoder's float32 rows, then log-probabilities
    const float *rows32 = nullptr;
    if (const int rc = align_lsm_rows(d, probs, seq_lens, B, T, V, stream, &rows32)) return rc;
    e->probs = rows32;
    e->dtype = CTCD_DTYPE_F32;
  }
  return CTCD_OK;
}

}  // namespace ctcalign

using namespace ctcalign;

extern "C" {

int ctcd_ctc_align(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *tokens,
                   const int32_t *lens, int R, int L_stride, int32_t *out_start, int32_t *out_end, float *out_scores, int32_t *status, void *stream) {
  ctcdev::DeviceGuard guard;
  AlignEntry en;
  const int rc = align_entry("ctcd_ctc_align", d, probs, seq_lens, B, T, V, blank_id, log_input, tokens, lens, R, L_stride,
                             out_scores && (L_stride == 0 || (out_start && out_end)), stream, &guard, &en);
  if (rc != CTCD_OK || en.rows == 0) return rc;
  const size_t slot = align_slot_bytes(T, L_stride);
  const long long grid = align_grid(en.rows, en.inf.budget, slot);
  void *scratch = nullptr;
  if (const int rc2 = align_scratch(d, (size_t)grid * slot, &scratch)) return rc2;
  align_note_grid(d, grid);
  // class 0 takes a group of four rows per workgroup at a time (at most the groups), the other classes one row
  const long long groups = align_groups(en.rows);
  const hipError_t e = ctclattice::launch_classes(en.dtype, log_input == 0, T, L_stride, [&](auto dt, auto prob, auto cls) {
    const long long g = decltype(cls)::value == 0 && grid > groups ? groups : grid;
    hipLaunchKernelGGL((ctc_align_kernel<decltype(dt)::value, decltype(prob)::value, decltype(cls)::value>), dim3((unsigned)g), dim3(kAlignThreads), 0,
                       (hipStream_t)stream, en.probs, seq_lens, T, V, blank_id, tokens, lens, R, L_stride, en.rows, (char *)scratch, slot, out_start, out_end, out_scores,
                       status);
  });
  return e == hipSuccess ? CTCD_OK : align_fail(CTCD_EHIP, (std::string("alignment: ") + hipGetErrorString(e)).c_str());
}

}  // extern "C"
