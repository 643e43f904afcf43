// posterior_long.hip -- the per-label CTC posteriors of posterior.h for rows of more states than a workgroup holds in registers
// (include/ctcdecode_amd.h "Label posteriors", ctcd_set_long_posteriors).  A translation unit of its own: posterior.hip's entry point
// launches it behind the register classes, and no other kernel sees it.
//   ctc_posterior_banded_kernel<DT, PROB, NPL>  the rows of more than W = 256 * NPL states, one per workgroup, in bands of W states
//                                               and blocks of F frames (posterior.h "long posteriors").  Pass 1 is the banded
//                                               log-likelihood walk (lattice_device.h walk_row_banded), which also keeps a of every
//                                               F-th frame: the checkpoints.  Pass 2 takes the blocks from the last to the first: (a)
//                                               the forward bands walk the block's frames again from the checkpoint before it and store
//                                               every frame's a into the block buffer; (b) the bands of the reversed labels walk the
//                                               block's frames in descending order from the carry row, which is b; behind each frame
//                                               an odd cell reads its a from the block buffer, forms g and updates its label's
//                                               accumulators.  Those live in registers during a band visit and in the slot between two.
//                                               Behind block 0 the lanes write their labels' outputs and the workgroup zeroes the tails.
// Every cell is the definition's and every label sees its frames in the order n - 1 .. 0, so the outputs carry the bits of the
// register kernels (posterior.hip) whatever W and F are.  Memory: plain vector stores; a __threadfence() and a barrier between two band
// visits; device-scope loads of what another thread or visit wrote.
#include <hip/hip_runtime.h>

#include "../../include/ctcdecode_amd.h"
#include "lattice_device.h"
#include "posterior.h"

namespace ctcpost {

using namespace ctcalign;

// exact_math.h's tables, staged into LDS by every workgroup (Tables::w: [0, 32) exp2f, [32, 48) logf invc, [48, 64) logf logc)
static __device__ const uint64_t kExpTab[32] = CTC_EXP2F_TAB;
static __device__ const double kLogInvc[16] = CTC_LOGF_INVC;
static __device__ const double kLogLogc[16] = CTC_LOGF_LOGC;

__device__ __forceinline__ float load_f32(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Pass 1 (walk_row_banded): loglik.hip's cell; behind the last frame of a block that has a block behind it, the lane's states into
// the block's checkpoint row (row r = a[(r + 1) F - 1], S floats by global state); behind the last frame the end rule.
template <int NPL> struct CheckpointRow {
  const uint64_t *tbl;
  float *ckpt;
  int S, F, n;
  float ll;
  int next;   // the next frame to keep, and its row
  float *row;
  float v[NPL];

  __device__ __forceinline__ float cell(int k, float lp, float stay, float p1, float p2, bool has2) {
    return v[k] = ctcloglik::cell_update(lp, stay, p1, has2 ? p2 : neg_inf(), tbl);
  }
  // walk_row_banded has no hook per band, so the frame hook itself starts a band's count.  That rests on two things: walk_band calls
  // frame() for t = 1, 2, .. n - 1 in turn and never for frame 0 (a banded row has n >= L >= 128, so t == 1 is reached in every band),
  // and the first frame to keep, F - 1, lies beyond it (posterior.h kPostMinBlock: F >= 8).
  __device__ __forceinline__ void frame(int t, int s0, int) {
    static_assert(kPostMinBlock > 2, "the first checkpoint frame must lie beyond frame 1");
    if (t == 1) {
      next = F - 1;
      row = ckpt;
    }
    if (t == next) {
      if (t + 1 < n) {
#pragma unroll
        for (int k = 0; k < NPL; ++k)
          if (s0 + k < S) row[s0 + k] = v[k];
      }
      next += F;
      row += S;
    }
  }
  __device__ __forceinline__ void frames_done() { __threadfence(); }
  __device__ __forceinline__ void finish(float a_last, float a_before, int L, int) { ll = ctcloglik::end_value(L, a_last, a_before, tbl); }
};

// Pass 2 (a) (walk_segment): the same cell; every frame's values of the lane's states into the block buffer, frame t's S floats at
// (t - lo) * S.
template <int NPL> struct BlockForward {
  const uint64_t *tbl;
  float *buf;
  int S, lo;
  float v[NPL];

  __device__ __forceinline__ void first(int k, float, float a) { v[k] = a; }
  __device__ __forceinline__ float cell(int k, float lp, float stay, float p1, float p2, bool has2) {
    return v[k] = ctcloglik::cell_update(lp, stay, p1, has2 ? p2 : neg_inf(), tbl);
  }
  __device__ __forceinline__ void frame(int t, int s0, int) {
    float *row = buf + (size_t)(t - lo) * S + s0;
#pragma unroll
    for (int k = 0; k < NPL; ++k)
      if (s0 + k < S) row[k] = v[k];
  }
};

// Pass 2 (b) (walk_segment with REV, on the reversed labels): the same cell, which is b.  posterior.hip's BackwardRow over a block:
// the lane's odd states are labels' (NL of them), the frame's a comes from the block buffer by the row's own state index, and the
// load for frame t - 1 is issued behind frame t's cells.
template <int NPL> struct BlockBackward {
  static constexpr int NL = NPL == 1 ? 1 : NPL / 2;
  const uint64_t *tbl;
  const float *buf;
  int S, lo;
  float ll;
  int t;          // the frame the next cells belong to
  float an[NL];   // its a of the lane's odd states (-inf: no such state)
  LabelAcc acc[NL];

  static __device__ __forceinline__ int odd_state(int s0, int j) { return NPL == 1 ? s0 : s0 + 2 * j + 1; }
  __device__ __forceinline__ bool labelled(int s0, int j) const {
    const int s = odd_state(s0, j);
    return (s & 1) && s < S;
  }
  __device__ __forceinline__ void load(int tt, int s0) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      an[j] = neg_inf();
      if (labelled(s0, j)) an[j] = load_f32(buf + (size_t)(tt - lo) * S + mirrored_state(S, odd_state(s0, j)));
    }
  }
  __device__ __forceinline__ void note(int k, float lp, float b) {
    if (NPL == 1 || (k & 1)) {
      const int j = NPL == 1 ? 0 : k >> 1;
      acc_update(acc[j], t, g_step(an[j], b, lp, ll, tbl), lp, tbl);
    }
  }
  __device__ __forceinline__ void first(int k, float lp, float b) { note(k, lp, b); }
  __device__ __forceinline__ float cell(int k, float lp, float stay, float p1, float p2, bool has2) {
    const float b = ctcloglik::cell_update(lp, stay, p1, has2 ? p2 : neg_inf(), tbl);
    note(k, lp, b);
    return b;
  }
  __device__ __forceinline__ void frame(int tt, int s0, int) {
    t = tt - 1;
    if (t >= lo) load(t, s0);
  }
};

// a label's accumulators in the slot: one 16-byte access
__device__ __forceinline__ void acc_store(LabelAcc *p, const LabelAcc &c) {
  ctclattice::i32x4 w;
  w.x = __float_as_int(c.occ);
  w.y = __float_as_int(c.num);
  w.z = __float_as_int(c.best);
  w.w = c.peak;
  *reinterpret_cast<ctclattice::i32x4 *>(p) = w;
}
__device__ __forceinline__ void acc_load(LabelAcc &c, const LabelAcc *p) {
  const ctclattice::i32x4 w = *reinterpret_cast<const ctclattice::i32x4 *>(p);
  c.occ = __int_as_float(w.x);
  c.num = __int_as_float(w.y);
  c.best = __int_as_float(w.z);
  c.peak = w.w;
}

// The rows of a launch (lattice_device.h walk_groups<-NPL>): only banded_row runs here; the other rows are the register classes'.
template <int DT, bool PROB> struct PosteriorLongRows {
  const uint64_t *tbl;
  const void *probs;
  int T, V, blank;
  const int32_t *tokens;
  int L_stride, F;
  char *slot;
  int32_t *out_pk;
  float *out_occ, *out_conf, *out_ll;

  __device__ __forceinline__ void zero_tails(size_t o, int from, int tid) {
    ctclattice::zero_words(out_pk + o + from, L_stride - from, tid, kAlignThreads);
    ctclattice::zero_words(reinterpret_cast<int32_t *>(out_occ + o) + from, L_stride - from, tid, kAlignThreads);
    ctclattice::zero_words(reinterpret_cast<int32_t *>(out_conf + o) + from, L_stride - from, tid, kAlignThreads);
  }

  template <int NPL> __device__ __forceinline__ void banded_row(long long row, int b, int n, int L, int tid) {
    constexpr int W = kAlignThreads * NPL, NL = BlockBackward<NPL>::NL;
    const int32_t *tok = tokens + (size_t)row * L_stride;
    const size_t o = (size_t)row * L_stride, row0 = (size_t)b * T;
    const int S = n_states(L), nb = band_count(S, W);
    LabelAcc *accs = reinterpret_cast<LabelAcc *>(slot + post_long_acc_offset());
    float *ckpt = reinterpret_cast<float *>(slot + post_long_ckpt_offset(T, L_stride, F));
    float *buf = reinterpret_cast<float *>(slot + post_long_buf_offset(T, L_stride, F));
    float *carry = reinterpret_cast<float *>(slot + post_long_carry_offset(T, L_stride, F));
    auto edge_col = [&](int j) { return slot + post_long_block_edge_offset(T, L_stride, F, j & 1); };

    // pass 1: ll, and the checkpoints
    CheckpointRow<NPL> f{tbl, ckpt, S, F, n, 0.0f, 0, ckpt, {}};
    ctclattice::walk_row_banded<NPL, DT, PROB>(f, probs, row0, n, T, V, blank, tok, L, tid, slot + post_long_edge_offset(T, L_stride, 0));
    if (tid == 0) out_ll[row] = f.ll;
    if (!(f.ll > neg_inf())) {  // (the same on every thread) no alignment: the outputs are 0
      zero_tails(o, 0, tid);
      return;
    }
    __threadfence();
    __syncthreads();

    // pass 2: the blocks from the last to the first
    const int last = (n - 1) / F;
    for (int k = last; k >= 0; --k) {
      const int lo = k * F, hi = (lo + F < n ? lo + F : n) - 1;
      // (a) a of the block's frames, from the checkpoint before it
      for (int j = 0; j < nb; ++j) {
        const int base = band_first_state(j, W), s0 = base + tid * NPL;
        float a[NPL];
        if (k > 0) {
          const float *ck = ckpt + (size_t)(k - 1) * S;
#pragma unroll
          for (int i = 0; i < NPL; ++i) a[i] = s0 + i < S ? load_f32(ck + s0 + i) : neg_inf();
        }
        BlockForward<NPL> fw{tbl, buf, S, lo, {}};
        ctclattice::walk_segment<NPL, DT, PROB, false>(fw, probs, row0, n, V, blank, ctclattice::RowLabels{tok}, S, base, k > 0 ? lo - 1 : 0, hi, k == 0, a,
                                                       j > 0 ? reinterpret_cast<const unsigned long long *>(edge_col(j - 1)) : nullptr,
                                                       j + 1 < nb ? reinterpret_cast<float2 *>(edge_col(j)) : nullptr, tid);
        __threadfence();
        __syncthreads();
      }
      // (b) b over the block's frames in descending order, from the carry row; the labels' accumulators
      for (int j = 0; j < nb; ++j) {
        const int base = band_first_state(j, W), s0 = base + tid * NPL;  // (states of the reversed labels)
        float bv[NPL];
        BlockBackward<NPL> bw{tbl, buf, S, lo, f.ll, hi, {}, {}};
        if (k < last) {
#pragma unroll
          for (int i = 0; i < NPL; ++i) bv[i] = s0 + i < S ? load_f32(carry + s0 + i) : neg_inf();
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          acc_init(bw.acc[i]);
          if (k < last && bw.labelled(s0, i)) acc_load(bw.acc[i], accs + (mirrored_state(S, bw.odd_state(s0, i)) >> 1));
        }
        bw.load(hi, s0);
        ctclattice::walk_segment<NPL, DT, PROB, true>(bw, probs, row0, n, V, blank, ctclattice::ReversedLabels{tok, L}, S, base, k < last ? n - 2 - hi : 0, n - 1 - lo,
                                                      k == last, bv, j > 0 ? reinterpret_cast<const unsigned long long *>(edge_col(j - 1)) : nullptr,
                                                      j + 1 < nb ? reinterpret_cast<float2 *>(edge_col(j)) : nullptr, tid);
        if (k > 0) {
#pragma unroll
          for (int i = 0; i < NPL; ++i)
            if (s0 + i < S) carry[s0 + i] = bv[i];
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
          if (bw.labelled(s0, i)) {
            const int lab = mirrored_state(S, bw.odd_state(s0, i)) >> 1;
            if (k > 0) {
              acc_store(accs + lab, bw.acc[i]);
            } else {
              out_pk[o + lab] = bw.acc[i].peak;
              out_occ[o + lab] = bw.acc[i].occ;
              out_conf[o + lab] = acc_confidence(bw.acc[i]);
            }
          }
        }
        __threadfence();
        __syncthreads();
      }
    }
    zero_tails(o, L, tid);
  }
  // (walk_groups names them for the classes this kernel is not)
  __device__ __forceinline__ void short_row(long long, int, int, int, int, int) {}
  template <int NPL> __device__ __forceinline__ void long_row(long long, int, int, int, int) {}
  template <int WAVES> __device__ __forceinline__ void no_row(long long, float, int) {}
};

template <int DT, bool PROB, int NPL>
__global__ void __launch_bounds__(kAlignThreads) ctc_posterior_banded_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens,
                                                                             const int32_t *lens, int R, int L_stride, long long rows, char *scratch, size_t slot_bytes,
                                                                             int F, int32_t *out_pk, float *out_occ, float *out_conf, float *out_ll, int32_t *status) {
  __shared__ uint64_t s_tbl[64];
  const int tid = (int)threadIdx.x;
  if (tid < 32) s_tbl[tid] = kExpTab[tid];
  else if (tid < 48) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogInvc[tid - 32]);
  else if (tid < 64) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogLogc[tid - 48]);
  // (the first barrier of the walk stands between these stores and their readers)
  PosteriorLongRows<DT, PROB> pol{s_tbl, probs, T, V, blank, tokens, L_stride, F, scratch + (size_t)blockIdx.x * slot_bytes, out_pk, out_occ, out_conf, out_ll};
  ctclattice::walk_groups<-NPL>(pol, seq_lens, T, V, blank, tokens, lens, R, L_stride, rows, status);
}

template <int DT, bool PROB, int NPL> static void launch(const PostLongLaunch &a, long long grid, void *stream) {
  hipLaunchKernelGGL((ctc_posterior_banded_kernel<DT, PROB, NPL>), dim3((unsigned)grid), dim3(kAlignThreads), 0, (hipStream_t)stream, a.probs, a.seq_lens, a.T, a.V,
                     a.blank, a.tokens, a.lens, a.R, a.L_stride, a.rows, a.scratch, a.slot_bytes, a.F, a.out_pk, a.out_occ, a.out_conf, a.out_ll, a.status);
}
template <int DT, bool PROB> static void launch_npl(int npl, const PostLongLaunch &a, long long grid, void *stream) {
  if (npl == 1) launch<DT, PROB, 1>(a, grid, stream);
  else if (npl == 4) launch<DT, PROB, 4>(a, grid, stream);
  else launch<DT, PROB, 16>(a, grid, stream);
}
template <int DT> static void launch_mode(bool prob, int npl, const PostLongLaunch &a, long long grid, void *stream) {
  prob ? launch_npl<DT, true>(npl, a, grid, stream) : launch_npl<DT, false>(npl, a, grid, stream);
}

void post_launch_banded(int dtype, bool prob, int npl, const PostLongLaunch &a, long long grid, void *stream) {
  if (dtype == CTCD_DTYPE_F16) launch_mode<ctcskip::kSkipF16>(prob, npl, a, grid, stream);
  else if (dtype == CTCD_DTYPE_BF16) launch_mode<ctcskip::kSkipBF16>(prob, npl, a, grid, stream);
  else launch_mode<ctcskip::kSkipF32>(prob, npl, a, grid, stream);
}

}  // namespace ctcpost
