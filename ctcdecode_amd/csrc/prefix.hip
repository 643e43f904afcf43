// prefix.hip -- the CTC prefix scores of prefix.h on the device, and their C ABI (include/ctcdecode_amd.h "CTC prefix scores").  A
// translation unit of its own, like loglik.hip.
//   ctc_prefix_scores_kernel<DT, PROB, STAGED, LISTED>  a workgroup of four waves per item, tile of prefixes and tile of candidates.  Its
//       lanes form groups of W = 32 .. 256, one candidate per lane, a group per hs prefixes.  Per chunk of F = 32 frames the workgroup
//       folds the prefixes' columns into LDS -- (r_b[t-1], phi_all[t-1]) per prefix and frame, one frame per lane, one lse3 each --
//       and then every lane walks the chunk alone, no barrier inside: it takes lp(t, c) once, and for each of its group's prefixes
//       one LDS broadcast, one addition and one (m, s) step.  With all labels as candidates (LISTED false) a lane's candidate is its
//       index, its loads are consecutive and one row value serves up to H = 8 prefixes from registers; with listed candidates every
//       prefix has a list of its own, so a group has one prefix and the loads are gathers.  STAGED (V <= 128): the chunk's rows go
//       through LDS, converted once; otherwise a lane loads its own column eight frames ahead.  The columns and rows of the next
//       chunk are in flight in registers while this one is walked.
//   ctc_prefix_advance_kernel<DT, PROB, INIT>  one wave per 64 new prefixes, one per lane, sequential over the frames: two independent
//       lse3 per frame.  The parents' columns come in and the children's go out through an LDS tile of 64 prefixes x 16 frames, so
//       that sixteen consecutive lanes move 128 consecutive bytes; a lane reads its parent's pair and writes its own in place.  The
//       gather from the parent slot is the tile's load.  INIT: no parent, the blank column's running sum into slot 0 of each item.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "prefix.h"

namespace ctcprefix {

using namespace ctcalign;
using ctcskip::clamped_len;
using ctcskip::kSkipBF16;
using ctcskip::kSkipF16;
using ctcskip::kSkipF32;
using ctcskip::widen_at;

constexpr int F = kPxChunk;

// exact_math.h's tables, staged into LDS by every workgroup (Tables::w: [0, 32) exp2f, [32, 48) logf invc, [48, 64) logf logc)
static __device__ const uint64_t kExpTab[32] = CTC_EXP2F_TAB;
static __device__ const double kLogInvc[16] = CTC_LOGF_INVC;
static __device__ const double kLogLogc[16] = CTC_LOGF_LOGC;
__device__ __forceinline__ void stage_tables(uint64_t *s_tbl, int tid) {
  if (tid < 32) s_tbl[tid] = kExpTab[tid];
  else if (tid < 48) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogInvc[tid - 32]);
  else if (tid < 64) s_tbl[tid] = (uint64_t)__double_as_longlong(kLogLogc[tid - 48]);
}
template <bool PROB> __device__ __forceinline__ float to_lp(float x) { return PROB ? prob_to_lp(x) : x; }

template <int DT, bool PROB, bool STAGED, bool LISTED>
__global__ void __launch_bounds__(kPxThreads) ctc_prefix_scores_kernel(const void *probs, const int32_t *seq_lens, int T, int V, int blank, const float2 *cols,
                                                                       const int32_t *last, const int32_t *lens, int R, const int32_t *cands, int C, int lg, int hs,
                                                                       float *out_scores, float *out_eos, int32_t *status) {
  constexpr int HS = LISTED ? 1 : kPxSlots;                     // (listed: hs == 1)
  constexpr int kPairs = kPxMaxWgSlots * F / kPxThreads;        // 8: pairs a thread folds per chunk at most
  constexpr int kRows = F * kPxStagedMaxV / kPxThreads;         // 16: row values a thread stages per chunk at most
  extern __shared__ __attribute__((aligned(16))) float s_row[];  // STAGED: lp(t0 + j, c) at j * V + c
  __shared__ uint64_t s_tbl[64];
  __shared__ float2 s_pp[kPxMaxWgSlots * F];  // (r_b[t-1], phi_all[t-1]) of the workgroup's prefix sl at frame t0 + j: sl * F + j
  __shared__ int s_code[kPxMaxWgSlots], s_last[kPxMaxWgSlots];
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, W = 1 << lg, g = tid >> lg, i = tid & (W - 1);
  const int SW = (kPxThreads >> lg) * hs, slot0 = (int)blockIdx.z * SW;  // the workgroup's prefixes: slot0 + [0, SW)
  const int n = clamped_len(seq_lens, b, T);
  const size_t row0 = (size_t)b * T, hyp0 = (size_t)b * R;

  stage_tables(s_tbl, tid);
  if (tid < SW) {
    const int slot = slot0 + tid;
    const int code = slot < R ? slot_code(lens[hyp0 + slot], last[hyp0 + slot], V, blank) : kSlotUnused;
    s_code[tid] = code;
    s_last[tid] = code >= 1 ? last[hyp0 + slot] : -1;
  }
  __syncthreads();

  // ---- the end scores, and a bad prefix's status: on the workgroups of the first candidate tile
  if (blockIdx.y == 0 && tid < SW && slot0 + tid < R) {
    const int code = s_code[tid];
    float eos = neg_inf();
    if (code >= 0) {
      if (n == 0) {
        eos = eos_no_frames(code);
      } else {
        const float2 p = cols[(hyp0 + slot0 + tid) * T + (size_t)(n - 1)];
        eos = eos_value(code, Pair{p.x, p.y}, s_tbl);
      }
    }
    out_eos[hyp0 + slot0 + tid] = eos;
    if (code == kSlotBad && status) status[b] = ALIGN_BAD_ROW;  // (raised only)
  }

  // ---- the lane's candidate, validated before the first frame; `col` is always a column of the row
  const int cidx = (int)blockIdx.y * W + i, gslot = slot0 + g * hs;  // the group's prefixes: gslot + [0, hs)
  const bool have = cidx < C && gslot < R;
  int c = -1;
  if (have) c = LISTED ? cands[(hyp0 + gslot) * C + (size_t)cidx] : cidx;
  const int ccode = cand_code(c, V, blank);
  if (have && ccode == kCandBad && status) status[b] = ALIGN_BAD_ROW;
  const int col = ccode == kCandOk ? c : blank;
  unsigned same = 0u;  // bit h: the candidate equals the last label of the group's prefix h
#pragma unroll
  for (int h = 0; h < HS; ++h)
    if (h < hs && s_code[g * hs + h] >= 1 && s_last[g * hs + h] == c) same |= 1u << h;
  Sum acc[HS];
#pragma unroll
  for (int h = 0; h < HS; ++h) acc[h] = sum_none();

  // ---- a chunk's inputs, loaded a chunk ahead: the columns' pairs at t - 1 (thread: frame tid & 31 of the prefixes (tid >> 5) + 8u),
  // and the staged rows
  float2 np[kPairs];
  float nx[STAGED ? kRows : 1];
  float nl[STAGED ? 1 : kPxAhead];
  const int pj = tid & (F - 1), psl = tid >> 5;
  auto prefetch = [&](int t0) {
    const int t = t0 + pj;
#pragma unroll
    for (int u = 0; u < kPairs; ++u) {
      const int sl = psl + (kPxThreads / F) * u;
      if (sl < SW && s_code[sl] >= 0 && t >= 1 && t < n) np[u] = cols[(hyp0 + slot0 + sl) * T + (size_t)(t - 1)];
    }
    if (STAGED) {
      const int cnt = (n - t0 < F ? n - t0 : F) * V;
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
        const int e = tid + kPxThreads * u;
        if (e < cnt) nx[u] = widen_at<DT>(probs, (row0 + (size_t)t0) * V + (size_t)e);
      }
    }
  };
  auto fold = [&](int t0) {  // the loaded chunk into LDS
    const int t = t0 + pj;
#pragma unroll
    for (int u = 0; u < kPairs; ++u) {
      const int sl = psl + (kPxThreads / F) * u;
      if (sl < SW) {
        float2 pp = make_float2(neg_inf(), neg_inf());
        const int code = s_code[sl];
        if (code >= 0 && t < n) {
          if (t == 0) pp.x = pp.y = phi_before_first(code);
          else pp = make_float2(np[u].y, phi_all(Pair{np[u].x, np[u].y}, s_tbl));
        }
        s_pp[sl * F + pj] = pp;
      }
    }
    if (STAGED) {
      const int cnt = (n - t0 < F ? n - t0 : F) * V;
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
        const int e = tid + kPxThreads * u;
        if (e < cnt) s_row[e] = to_lp<PROB>(nx[u]);
      }
    }
  };
  // gathered rows: the lane's own column at the frames [t, t + kPxAhead)
  auto fetch = [&](int t) {
#pragma unroll
    for (int k = 0; k < kPxAhead; ++k)
      if (t + k < n) nl[STAGED ? 0 : k] = widen_at<DT>(probs, (row0 + (size_t)(t + k)) * V + (size_t)col);
  };
  auto step = [&](float lp, int j) {
#pragma unroll
    for (int h = 0; h < HS; ++h)
      if (h < hs) {
        const float2 pp = s_pp[(g * hs + h) * F + j];
        sum_step(acc[h], lp + ((same >> h) & 1u ? pp.x : pp.y), s_tbl);
      }
  };

  // a lane without a candidate to score (beyond C or R, -1, the blank, invalid) folds and stages with the others and walks nothing
  const bool live = have && ccode == kCandOk;
  if (n > 0) {
    prefetch(0);
    if (!STAGED && live) fetch(0);
  }
  for (int t0 = 0; t0 < n; t0 += F) {
    const int fr = n - t0 < F ? n - t0 : F;
    fold(t0);
    __syncthreads();
    if (t0 + F < n) prefetch(t0 + F);  // (in flight while this chunk is walked)
    if (!live) {
    } else if (STAGED) {
      for (int j = 0; j < fr; ++j) step(s_row[j * V + col], j);
    } else {
      for (int j0 = 0; j0 < fr; j0 += kPxAhead) {
        float cl[kPxAhead];
#pragma unroll
        for (int k = 0; k < kPxAhead; ++k) cl[k] = to_lp<PROB>(nl[STAGED ? 0 : k]);
        fetch(t0 + j0 + kPxAhead);
#pragma unroll
        for (int k = 0; k < kPxAhead; ++k)
          if (j0 + k < fr) step(cl[k], j0 + k);
      }
    }
    __syncthreads();  // (the chunk is walked: its LDS is free)
  }

  if (have) {
#pragma unroll
    for (int h = 0; h < HS; ++h)
      if (h < hs && gslot + h < R) out_scores[(hyp0 + gslot + h) * C + (size_t)cidx] = ccode == kCandOk ? sum_final(acc[h], s_tbl) : neg_inf();
  }
}

// hypothesis q = b * Rn + j of the launch: INIT: slot j of item b (slot 0 runs, the others are marked unused); else child j of item b
template <int DT, bool PROB, bool INIT>
__global__ void __launch_bounds__(kPxAdvThreads) ctc_prefix_advance_kernel(const void *probs, const int32_t *seq_lens, long long hyps, int T, int V, int blank,
                                                                           const float2 *pcols, const int32_t *plast, const int32_t *plens, int R,
                                                                           const int32_t *parents, const int32_t *labels, int Rn, float2 *ccols, int32_t *clast,
                                                                           int32_t *clens, int32_t *status) {
  constexpr int FA = kPxAdvFrames, kStride = FA + 1;  // (a prefix's tile row: 17 pairs, so that the lanes' rows start in different banks)
  __shared__ uint64_t s_tbl[64];
  __shared__ float2 s_tile[kPxAdvThreads * kStride];
  __shared__ long long s_src[kPxAdvThreads];  // the parent's first pair, or -1
  __shared__ int s_n[kPxAdvThreads];          // the frames a lane's prefix runs (0: none)
  const int lane = (int)threadIdx.x;
  const long long q = (long long)blockIdx.x * kPxAdvThreads + lane;
  stage_tables(s_tbl, lane);

  // ---- the lane's prefix, validated before the first frame
  bool act = false, differs = true, parent_empty = true;
  int n = 0, c = blank;
  long long src = -1;
  size_t row0 = 0;
  if (q < hyps) {
    const int b = (int)(q / Rn), j = (int)(q % Rn);
    row0 = (size_t)b * T;
    int len = -1, lst = -1;
    if (INIT) {
      act = j == 0;
      len = act ? 0 : -1;
    } else {
      const int p = parents[q];
      c = labels[q];
      bool ok = p >= 0 && p < R && label_ok(c, V, blank);
      int pcode = kSlotBad;
      if (ok) {
        pcode = slot_code(plens[(size_t)b * R + p], plast[(size_t)b * R + p], V, blank);
        ok = pcode >= 0;
      }
      if (ok) {
        act = true;
        len = pcode + 1;
        lst = c;
        parent_empty = pcode == 0;
        differs = parent_empty || c != plast[(size_t)b * R + p];
        src = (long long)((size_t)b * R + p) * T;
      } else {
        c = blank;  // (always a column of the row)
        if (p != -1 && status) status[b] = ALIGN_BAD_ROW;  // (raised only; p == -1: an unused slot)
      }
    }
    clens[q] = len;
    clast[q] = lst;
    if (act) n = clamped_len(seq_lens, b, T);
  }
  s_src[lane] = src;
  s_n[lane] = n;
  __syncthreads();

  // ---- a tile's inputs, loaded a tile ahead: the parents' pairs (thread: frame lane & 15 of the prefixes (lane >> 4) + 4k) and the
  // lane's own two columns of the rows
  float2 tp[FA];
  float lc[INIT ? 1 : FA], lb[FA];
  const int part = lane & (FA - 1), hq = lane >> 4;
  auto prefetch = [&](int t0) {
    if (!INIT) {
#pragma unroll
      for (int k = 0; k < FA; ++k) {
        const int h = hq + (kPxAdvThreads / FA) * k;
        if (s_src[h] >= 0 && t0 + part < s_n[h]) tp[k] = pcols[s_src[h] + t0 + part];
      }
    }
#pragma unroll
    for (int k = 0; k < FA; ++k)
      if (t0 + k < n) {
        if (!INIT) lc[INIT ? 0 : k] = widen_at<DT>(probs, (row0 + (size_t)(t0 + k)) * V + (size_t)c);
        lb[k] = widen_at<DT>(probs, (row0 + (size_t)(t0 + k)) * V + (size_t)blank);
      }
  };
  Pair ch{neg_inf(), neg_inf()}, pa{neg_inf(), neg_inf()};
  if (__any(n > 0)) prefetch(0);
  for (int t0 = 0; __any(t0 < n); t0 += FA) {
    if (!INIT) {
#pragma unroll
      for (int k = 0; k < FA; ++k) s_tile[(hq + (kPxAdvThreads / FA) * k) * kStride + part] = tp[k];
    }
    float cc[INIT ? 1 : FA], cb[FA];
#pragma unroll
    for (int k = 0; k < FA; ++k) {
      if (!INIT) cc[INIT ? 0 : k] = to_lp<PROB>(lc[INIT ? 0 : k]);
      cb[k] = to_lp<PROB>(lb[k]);
    }
    __syncthreads();
    if (__any(t0 + FA < n)) prefetch(t0 + FA);  // (in flight while this tile is walked)
#pragma unroll
    for (int k = 0; k < FA; ++k) {
      const int t = t0 + k;
      if (t < n) {
        if (INIT) {
          ch = t == 0 ? init_first(cb[k]) : init_cell(cb[k], ch, s_tbl);
        } else {
          const float2 p = s_tile[lane * kStride + k];  // the parent's pair at t: read before the child's takes its place
          ch = t == 0 ? advance_first(cc[INIT ? 0 : k], parent_empty) : advance_cell(cc[INIT ? 0 : k], cb[k], ch, pa, differs, s_tbl);
          pa = Pair{p.x, p.y};
        }
        s_tile[lane * kStride + k] = make_float2(ch.n, ch.b);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FA; ++k) {
      const int h = hq + (kPxAdvThreads / FA) * k;
      const long long hq_q = (long long)blockIdx.x * kPxAdvThreads + h;
      if (t0 + part < s_n[h]) ccols[(size_t)hq_q * T + (size_t)(t0 + part)] = s_tile[h * kStride + part];
    }
    __syncthreads();
  }
}

template <typename Fn> void by_dtype(int dt, Fn fn) {
  if (dt == kSkipF16) fn(std::integral_constant<int, kSkipF16>());
  else if (dt == kSkipBF16) fn(std::integral_constant<int, kSkipBF16>());
  else fn(std::integral_constant<int, kSkipF32>());
}
template <typename Fn> void by_flag(bool v, Fn fn) {
  if (v) fn(std::true_type());
  else fn(std::false_type());
}

// What the three entry points do alike before their launch: ctcd_ctc_loglik's checks (align_entry, without label rows), then -> the
// rows to read and their dtype code
int prefix_entry(const char *fn, ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const int32_t *lens,
                 int R, bool outputs, void *stream, ctcdev::DeviceGuard *guard, AlignEntry *en, int *dt) {
  const int rc = align_entry(fn, d, probs, seq_lens, B, T, V, blank_id, log_input, nullptr, lens, R, 0, outputs, stream, guard, en);
  if (rc != CTCD_OK || en->rows == 0) return rc;
  *dt = en->dtype == CTCD_DTYPE_F16 ? kSkipF16 : (en->dtype == CTCD_DTYPE_BF16 ? kSkipBF16 : kSkipF32);
  return CTCD_OK;
}
int launched(const char *what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CTCD_OK : align_fail(CTCD_EHIP, (std::string(what) + hipGetErrorString(e)).c_str());
}

}  // namespace ctcprefix

using namespace ctcprefix;

extern "C" {

int ctcd_ctc_prefix_init(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, int R, float *out_cols,
                         int32_t *out_last, int32_t *out_lens, void *stream) {
  ctcdev::DeviceGuard guard;
  AlignEntry en;
  int dt = 0;
  const int rc = prefix_entry("ctcd_ctc_prefix_init", d, probs, seq_lens, B, T, V, blank_id, log_input, out_lens, R, out_last && (T == 0 || out_cols), stream, &guard,
                              &en, &dt);
  if (rc != CTCD_OK || en.rows == 0) return rc;
  const bool prob = log_input == 0;
  const unsigned grid = (unsigned)((en.rows + kPxAdvThreads - 1) / kPxAdvThreads);
  by_dtype(dt, [&](auto tdt) {
    by_flag(prob, [&](auto tprob) {
      hipLaunchKernelGGL((ctc_prefix_advance_kernel<decltype(tdt)::value, decltype(tprob)::value, true>), dim3(grid), dim3(kPxAdvThreads), 0, (hipStream_t)stream,
                         en.probs, seq_lens, en.rows, T, V, blank_id, (const float2 *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr, 0,
                         (const int32_t *)nullptr, (const int32_t *)nullptr, R, (float2 *)out_cols, out_last, out_lens, (int32_t *)nullptr);
    });
  });
  prefix_note_kernel(d, px_kernel_code(kPxKindInit, dt, prob, false, false, 0, 0));
  return launched("prefix init: ");
}

int ctcd_ctc_prefix_scores(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const float *cols,
                           const int32_t *last, const int32_t *lens, int R, const int32_t *candidates, int C, float *out_scores, float *out_eos, int32_t *status,
                           void *stream) {
  ctcdev::DeviceGuard guard;
  AlignEntry en;
  int dt = 0;
  const bool listed = candidates != nullptr;
  if (listed && C < 0) return align_fail(CTCD_EINVAL, "ctcd_ctc_prefix_scores: C >= 0 required");
  if (!listed) C = V;  // (V is checked below, before C is used)
  const int rc = prefix_entry("ctcd_ctc_prefix_scores", d, probs, seq_lens, B, T, V, blank_id, log_input, lens, R,
                              last && out_eos && (C == 0 || out_scores) && (T == 0 || cols), stream, &guard, &en, &dt);
  if (rc != CTCD_OK || en.rows == 0) return rc;
  const bool prob = log_input == 0, staged = px_staged(V);
  const int lg = px_group_log2(C), hs = px_group_slots(listed, R, lg), per_wg = (kPxThreads >> lg) * hs;
  const long long ytiles = C == 0 ? 1 : ((long long)C + (1 << lg) - 1) >> lg, ztiles = ((long long)R + per_wg - 1) / per_wg;
  if (ytiles > 65535 || ztiles > 65535) return align_fail(CTCD_EUNSUPPORTED, "ctcd_ctc_prefix_scores: too many candidates or prefixes for one launch");
  const dim3 grid((unsigned)B, (unsigned)ytiles, (unsigned)ztiles);
  by_dtype(dt, [&](auto tdt) {
    by_flag(prob, [&](auto tprob) {
      by_flag(staged, [&](auto tst) {
        by_flag(listed, [&](auto tli) {
          hipLaunchKernelGGL((ctc_prefix_scores_kernel<decltype(tdt)::value, decltype(tprob)::value, decltype(tst)::value, decltype(tli)::value>), grid,
                             dim3(kPxThreads), px_lds_bytes(V), (hipStream_t)stream, en.probs, seq_lens, T, V, blank_id, (const float2 *)cols, last, lens, R,
                             candidates, C, lg, hs, out_scores, out_eos, status);
        });
      });
    });
  });
  prefix_note_kernel(d, px_kernel_code(kPxKindScores, dt, prob, staged, listed, lg, hs));
  return launched("prefix scores: ");
}

int ctcd_ctc_prefix_advance(ctcd_decoder *d, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input, const float *cols,
                            const int32_t *last, const int32_t *lens, int R, const int32_t *parents, const int32_t *labels, int R_new, float *out_cols,
                            int32_t *out_last, int32_t *out_lens, int32_t *status, void *stream) {
  ctcdev::DeviceGuard guard;
  AlignEntry en;
  int dt = 0;
  if (R < 0) return align_fail(CTCD_EINVAL, "ctcd_ctc_prefix_advance: R >= 0 required");
  const int rc = prefix_entry("ctcd_ctc_prefix_advance", d, probs, seq_lens, B, T, V, blank_id, log_input, out_lens, R_new,
                              parents && labels && out_last && (T == 0 || out_cols) && (R == 0 || (last && lens && (T == 0 || cols))), stream, &guard, &en, &dt);
  if (rc != CTCD_OK || en.rows == 0) return rc;
  const bool prob = log_input == 0;
  const unsigned grid = (unsigned)((en.rows + kPxAdvThreads - 1) / kPxAdvThreads);
  by_dtype(dt, [&](auto tdt) {
    by_flag(prob, [&](auto tprob) {
      hipLaunchKernelGGL((ctc_prefix_advance_kernel<decltype(tdt)::value, decltype(tprob)::value, false>), dim3(grid), dim3(kPxAdvThreads), 0, (hipStream_t)stream,
                         en.probs, seq_lens, en.rows, T, V, blank_id, (const float2 *)cols, last, lens, R, parents, labels, R_new, (float2 *)out_cols, out_last,
                         out_lens, status);
    });
  });
  prefix_note_kernel(d, px_kernel_code(kPxKindAdvance, dt, prob, false, false, 0, 0));
  return launched("prefix advance: ");
}

}  // extern "C"
