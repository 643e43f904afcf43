// lattice_device.h -- the walk over a CTC lattice that the forced alignment (align.hip) and the log-likelihood (loglik.hip) share on
// the device: how a hypothesis' extended sequence (align.h: S = 2L + 1 states) lies over the lanes of a wave or a workgroup and moves
// from frame to frame (walk_row), how the rows of a launch are validated, classed in groups of four and handed out (walk_groups),
// which kernels a shape needs (launch_classes), and how a unit zeroes the tail of an output row (zero_words).  The label posteriors
// (posterior.hip) walk a row twice with it, forward and -- on the reversed labels, the frames in descending order -- backward.  What
// a cell computes, what is kept of a frame and what follows the last one is the user's: a policy type each.  Device code with wave
// intrinsics: only those three files include it; what defines a result stays CTC_HD code in align.h / loglik.h / posterior.h, where
// the host twins compile it.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/ctcdecode_amd.h"
#include "align.h"

namespace ctclattice {

using namespace ctcalign;

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

// One hypothesis on one unit: WAVES = 1 (a wave, utid = its lane) or kAlignWaves (the workgroup, utid = the thread), NPL states per
// lane -- lane u holds states u * NPL .. u * NPL + NPL - 1 in registers, so that the neighbours s - 1 and s - 2 of all but a lane's
// first two states are its own.  The others come from the lane before it (__shfl_up) and, at a wave's first lane, from the wave before
// it through LDS (s_xch: two floats per wave and frame parity, written behind each frame, one barrier per frame).  A frame's NPL cells of
// a lane read only the frame before.  The row was validated by the caller: 0 <= L <= n, n >= 1, S = 2L + 1 <= 64 * WAVES * NPL, every
// label in [0, V) and no blank.  The policy P:
//   float cell(int k, float lp, float stay, float p1, float p2, bool has2)   the new value of the lane's k-th state from frame t - 1's
//                                  values of the state, of s - 1 and of s - 2 (has2: s - 2 is an allowed predecessor)
//   void frame(int t, int s0, int lane)                                      behind frame t's cells of the lane (first state s0)
//   void frames_done()                                                        behind the last frame
//   void finish(float last, float before, int L, int utid)                   with frame n - 1's states S - 1 and S - 2 (S - 2 is looked
//                                                                            at only if L >= 1), on every thread of the unit
// REV: the walk takes the item's frames in descending order, n - 1 first (`t` of the hooks is the frame itself; "frame t - 1" above is
// then frame t + 1) -- on the reversed labels that is the backward recurrence (posterior.hip).  FIRST: the policy also sees the walk's
// first frame, which no cell() computes:
//   void first(int k, float lp, float v)                                     the lane's k-th state of the first frame: its lp, and its
//                                                                            value v (-inf for all but the first two states)
// followed by frame() for that frame.  Both default to what align.hip and loglik.hip were written for.
template <int WAVES, int NPL, int DT, bool PROB, bool REV = false, bool FIRST = false, class P>
__device__ __forceinline__ void walk_row(P &pol, const void *probs, size_t row0, int n, int V, int blank, const int32_t *tok, int L, int utid) {
  constexpr int CH = NPL == 1 ? 8 : (NPL == 4 ? 4 : 2);  // frames whose log-probabilities are in flight while a chunk is computed
  const int lane = utid & 63, wave = utid >> 6;
  const int S = n_states(L), s0 = utid * NPL;
  __shared__ float s_xch[2 * kAlignWaves * 2], s_fin[2];  // (WAVES > 1; the caller's barrier behind the row frees them for the next one)
  float *xch = s_xch, *fin = s_fin;
  // the lane's states: the column each gathers, and which of them have the third predecessor (frame-invariant).  States at or beyond
  // S gather the blank's column and compute on: no state below them ever reads them, and what follows the last frame looks below them.
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
    const int tt = t < n ? t : n - 1;
    const char *fr = (const char *)probs + (row0 + (size_t)(REV ? n - 1 - tt : tt)) * (size_t)V * kElem;
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
  float a[NPL];
  auto publish = [&](int par) {
    if (WAVES > 1) {
      const float before = NPL >= 2 ? a[NPL >= 2 ? NPL - 2 : 0] : __shfl_up(a[0], 1, 64);
      if (lane == 63) {
        xch[(par * WAVES + wave) * 2] = a[NPL - 1];
        xch[(par * WAVES + wave) * 2 + 1] = before;
      }
      __syncthreads();
    }
  };

  float cur[CH][NPL], nxt[CH][NPL];
  load(cur[0], 0);
  convert(cur[0]);
#pragma unroll
  for (int k = 0; k < NPL; ++k) a[k] = (s0 + k < 2 && s0 + k < S) ? cur[0][k] : neg_inf();
  if constexpr (FIRST) {
#pragma unroll
    for (int k = 0; k < NPL; ++k) pol.first(k, cur[0][k], a[k]);
    pol.frame(REV ? n - 1 : 0, s0, lane);
  }
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
          a_in = __shfl_up(a[0], 1, 64);
          b_in = __shfl_up(a[0], 2, 64);
        } else {
          a_in = __shfl_up(a[NPL - 1], 1, 64);
          b_in = __shfl_up(a[NPL >= 2 ? NPL - 2 : 0], 1, 64);
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
#pragma unroll
        for (int k = NPL - 1; k >= 0; --k) {  // (descending: a[k - 1] and a[k - 2] are still frame t - 1's)
          const float p1 = k >= 1 ? a[k >= 1 ? k - 1 : 0] : a_in;
          const float p2 = k >= 2 ? a[k >= 2 ? k - 2 : 0] : (k == 1 ? a_in : b_in);
          a[k] = pol.cell(k, cur[c][k], a[k], p1, p2, (has2 >> k) & 1u);
        }
        pol.frame(REV ? n - 1 - t : t, s0, lane);
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
  // frame n - 1's states S - 1 and S - 2, from the lanes that hold them
  float mine1 = 0.0f, mine2 = 0.0f;
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    if (s0 + k == S - 1) mine1 = a[k];
    if (s0 + k == S - 2) mine2 = a[k];
  }
  pol.frames_done();
  float last, before = 0.0f;
  if (WAVES > 1) {
    if (s0 <= S - 1 && S - 1 < s0 + NPL) fin[0] = mine1;
    if (s0 <= S - 2 && S - 2 < s0 + NPL) fin[1] = mine2;
    __syncthreads();
    last = fin[0];
    if (L >= 1) before = fin[1];
  } else {
    last = __shfl(mine1, (S - 1) / NPL, 64);
    if (L >= 1) before = __shfl(mine2, (S - 2) / NPL, 64);
  }
  pol.finish(last, before, L, utid);
}

// The rows fall into four classes, and each class has a kernel of its own (CLS), so that each gets the registers its class needs and
// no more: 0 = the rows of a group of four consecutive rows that all fit a wave (S <= 64, and the rows that run no recurrence), one
// per wave side by side without a barrier (workgroup g takes the groups g, g + grid, ...); 1 / 4 / 16 = the rows of every other group,
// on the whole workgroup with that many states per lane (workgroup g takes the rows g, g + grid, ...; rows of such a group that run no
// recurrence: class 1).  Every kernel walks all rows and classes their groups alike; a row is written by exactly one of them.  A
// length outside [0, L_stride], a label outside [0, V) or equal to the blank makes a row invalid and raises its item's status word.
// The policy P, with row = the row's index in the launch, b = its item, n = the item's frames, L = its labels:
//   void short_row(long long row, int b, int n, int L, int lane, int wave)        run the row on this wave (S <= 64)
//   template <int NPL> void long_row(long long row, int b, int n, int L, int tid) run the row on the workgroup, NPL states per lane
//   template <int WAVES> void no_row(long long row, float score, int utid)        a row that runs no recurrence: its score is given
template <int CLS, class P>
__device__ __forceinline__ void walk_groups(P &pol, const int32_t *seq_lens, int T, int V, int blank, const int32_t *tokens, const int32_t *lens, int R,
                                            int L_stride, long long rows, int32_t *status) {
  __shared__ int s_row[kAlignWaves];  // what each wave found out about its row of the group
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
      what = row_code(ok, len, ctcskip::clamped_len(seq_lens, b, T));
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
        if (what < 0)
          pol.template no_row<1>(h, no_row_score(what, lens[h], n), lane);
        else
          pol.short_row(h, b, n, what, lane, wave);
      }
    } else if (!all_short) {
      const int code = s_row[(int)(u % kAlignWaves)];
      const int b = (int)(u / R), n = ctcskip::clamped_len(seq_lens, b, T);
      if (code < 0) {
        if (CLS == 1) pol.template no_row<kAlignWaves>(u, no_row_score(code, lens[u], n), tid);
      } else if (align_npl(n_states(code)) == CLS) {  // (the entry points refuse shapes whose rows can exceed kAlignMaxStates)
        pol.template long_row<CLS == 0 ? 1 : CLS>(u, b, n, code, tid);
      }
    }
    __syncthreads();  // (s_row and whatever else the unit used belong to the next unit)
  }
}

// The kernels a launch needs, one behind the other on the stream: f(DT, PROB, CLS) -- std::integral_constant values of the kernels'
// template arguments -- for the input's element type and mode and every class the shape allows (S <= 2 * min(L_stride, T) + 1).
template <int N> using Int = std::integral_constant<int, N>;
template <class F> hipError_t launch_classes(int dtype, bool prob, int T, int L_stride, F &&f) {
  const int smax = n_states(align_lmax(T, L_stride));
  auto classes = [&](auto dt, auto pr) {
    f(dt, pr, Int<0>());
    if (smax > 64) f(dt, pr, Int<1>());
    if (smax > kAlignThreads) f(dt, pr, Int<4>());
    if (smax > kAlignThreads * 4) f(dt, pr, Int<16>());
  };
  auto modes = [&](auto dt) { prob ? classes(dt, std::true_type()) : classes(dt, std::false_type()); };
  if (dtype == CTCD_DTYPE_F16) modes(Int<ctcskip::kSkipF16>());
  else if (dtype == CTCD_DTYPE_BF16) modes(Int<ctcskip::kSkipBF16>());
  else modes(Int<ctcskip::kSkipF32>());
  return hipGetLastError();
}

}  // namespace ctclattice
