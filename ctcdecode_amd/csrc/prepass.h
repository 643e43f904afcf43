// prepass.h -- what the library's host file needs of the pre-pass kernels (prepass.hip): the passes that run in front of the decode
// kernel on the caller's rows.  Those are the elementwise prob -> log and half -> float32 passes, the log-softmax of raw logits, the
// vocabulary prune (get_pruned_log_probs, decoder_utils.cpp:10-45) with its std::sort replay, and the launch-order pass.  The kernels
// themselves are in prepass.hip's unnamed namespace; the host reaches them through the table below (their addresses) and through
// launch_order, and sizes their launches with the constants and layout functions here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace {
// The argument block of the prune kernels.  (In the unnamed namespace, as the kernels that take it by value are: the host file fills
// its own copy of this one layout and hands it to hipLaunchKernel by address.)
struct PruneArgs {
  const float *in;          // [B, T, V]
  const int32_t *seq_lens;  // [B] or null
  int T, V, top_n, log_input, stride;
  long long rows;           // B * T
  double cutoff_prob;
  int *cnt, *ch;
  float *lp;
  unsigned *n_flag, *flag_rows;
  unsigned flag_cap;
  double cut_exp;            // exp(cutoff_prob)
  const uint64_t *tables;    // exact_math.h Tables, in global memory
  float *row_max, *row_lse;  // log_input == 2 (raw logits, prune_logits_wg_kernel): every frame's maximum and logf(sum of exponentials)
};
}  // namespace

namespace ctcprepass {

constexpr int kPruneCand = 256;  // capacity of the pre-filter candidate list per frame

// prune_resolve_kernel: its workgroup, the vocabulary its 16-bit positions cover, and the bytes its sort needs (in LDS, or per
// workgroup in global memory)
__host__ __device__ inline int prune_resolve_task_cap(int V) { return V / 17 + 2; }
constexpr int kResolveThreads = 1024;  // (the row fills most of a CU's LDS: one workgroup per CU whatever its size)
constexpr int kResolveMaxV = 65535;    // 16-bit positions and counters
__host__ __device__ inline size_t prune_resolve_lds_bytes(int V, int n) {
  // pairs | Lp, Rp | two task lists | final ranges | stack of long ranges | counters | the kept labels
  return (size_t)V * 8 + (size_t)2 * (V + 2) * 2 + (size_t)6 * prune_resolve_task_cap(V) * 2 + (size_t)2 * (V / 2 + 1) * 2 + 3 * 64 * 4 + 64 +
         (size_t)n * 4 + 64;
}

// the launch-order kernels: the bitonic sort's workgroup and the largest batch it takes; the rank kernel's workgroup
constexpr int kOrderThreads = 1024, kOrderSortMax = 16384;
constexpr int kOrderRankThreads = 256;

// ---- what prepass.hip exports to the library's host file (ctcdecode_amd.hip) -------------------------------------------------------
// Every pre-pass instantiation the build compiles, one row each: the kernel (CTCD_PP_*, include/ctcdecode_amd.h), its size parameter
// (F4 of the workgroup kernels, R of prune_rows_kernel, else 0), REG of prune_rows_wg_kernel (else 0), the input dtype, and the largest
// V the dispatch sends to it (0: no bound).  The dispatch picks from this table (pp_pick: the first row that takes V) and
// ctcd_debug_last_prepass reports from it, so the two cannot disagree.
struct PrepassEntry { const void *fn; int32_t kernel, a, b, dt, vmax; };
extern const PrepassEntry kPrepass[];
extern const int kPrepassCount;
// the first row of kernel `k` with REG `b` for dtype `dt` that takes V; null: none
const PrepassEntry *pp_pick(int k, int b, int dt, int V);
const PrepassEntry *pp_find(const void *fn);

// the launch-order pass (ctcd_set_launch_order) on `stream`: order = [ticket | permutation of the B items, longest first] from lens
// [B] (null: every item has T frames), both readable by the device.  One workgroup sorts batches of up to kOrderSortMax items whose
// keys fit max_lds bytes of LDS; larger ones are ranked.
hipError_t launch_order(const int32_t *lens, int B, int T, int max_lds, int *order, hipStream_t stream);

}  // namespace ctcprepass
