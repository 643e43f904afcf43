// launch_plan.h -- which decode kernel a call launches, with how many threads and how much LDS.  A pure function of the shape, the
// decoder's switches and two device limits, without HIP: the host code of ctcdecode_amd.hip runs it in front of everything a call
// queues, and the CPU suite runs it for every instantiation (tests/native/core_host.cpp ctccore_plan_kernel).  Which kernels exist
// is the build's CTC_KERNEL_LIST (decode_kernel.h), the one record of the instantiations: the caller hands it in.
#pragma once
#include <cmath>
#include <cstddef>
#include <string>

#include "../../include/ctcdecode_amd.h"
#include "beam_core.h"

namespace ctcdk {

// The template arguments of ctc_beam_decode_kernel (decode_kernel.h): PROF, BIG, LAYOUT, PRUNED, NT, LM (0 / 1 / 2 / 3), OCC2.
struct KernelKey {
  int prof, big, layout, pruned, nt, lm, occ2;
};
constexpr bool operator==(const KernelKey &a, const KernelKey &b) {
  return a.prof == b.prof && a.big == b.big && a.layout == b.layout && a.pruned == b.pruned && a.nt == b.nt && a.lm == b.lm && a.occ2 == b.occ2;
}
// The north-star class's default builds do not poll KernelArgs::frames_ready (decode_kernel.h kNoStreamedInput): with streamed rows
// their twins PROF 4 / 5 (of PROF 0 / 3) run instead.
CTC_HD constexpr bool ignores_streamed_input(const KernelKey &k) {
  return (k.prof == 0 || k.prof == 3) && k.layout == 1 && k.nt == 1024 && (k.lm == 0 || k.lm == 2) && !k.pruned && k.big == 0 && (!k.occ2 || k.lm == 0);
}
// The wide-beam run-time layouts (BIG at LAYOUT 0) take no launch order (decode_kernel.h kTicket): they keep batch order.
CTC_HD constexpr bool takes_launch_order(const KernelKey &k) { return !(k.big != 0 && k.layout == 0); }
// ctcd_debug_last_layout of a kernel: LAYOUT 3 -> 3, BIG b at LAYOUT 0 -> 3 + b (the HBM-scratch levels), otherwise LAYOUT.
constexpr int layout_of(const KernelKey &k) { return k.layout == 3 ? 3 : (k.big && k.layout == 0) ? 3 + k.big : k.layout; }

// The cutoff_prob the pre-passes and the workspace are built for.  The reference runs its cumulative cut only when
// log(cutoff_prob) < 0.0 (decoder_utils.cpp:16,21): not for a negative or NaN cutoff_prob, whose logarithm is NaN, nor for 1 or more.
// Every such value means "no cumulative cut", which the kernels and make_dims read as cutoff_prob == 1.0.
inline double used_cutoff_prob(double cutoff_prob) { return std::log(cutoff_prob) < 0.0 ? cutoff_prob : 1.0; }

inline ctcbeam::Dims make_dims(int beam, int V, int cutoff_top_n, double cutoff_prob, bool lm = false) {
  const bool pruned = cutoff_prob < 1.0 || cutoff_top_n < V;
  ctcbeam::Dims d;
  d.K = beam;
  d.V = V;
  d.Vc_max = pruned ? (cutoff_top_n < V ? cutoff_top_n : V) : V;
  d.use_rank_table = pruned ? 1 : 0;
  d.lm = lm ? 1 : 0;
  return d;
}

// The scorer of a call, as far as the choice goes: none; one whose builds serve any model (LM 1); a word model over at most 64 labels,
// which the LM 2 builds serve in the fixed layout (beam_core.h WORDLM; not with CTCD_GENERAL_LM_KERNEL=1); a callback (LM 3).
// Each value is the LM argument of the scorer's fixed-layout builds.
enum ScorerKind { kNoScorer = 0, kGeneralScorer = 1, kWordScorer = 2, kCallbackScorer = 3 };

// The decoder's switches the choice reads (ctcd_decoder; -1 = automatic for the two modes).
struct LaunchSwitches {
  bool no_fixed_layout, profile, tl_armed;
  int cu_sharing, subtree_mode;
  bool subtree_on;
};

struct LaunchPlan {
  KernelKey key;
  int threads;
  size_t lds, far_bytes;  // dynamic LDS of a workgroup; HBM scratch per utterance (a multiple of 256)
  int rc = CTCD_OK;       // or CTCD_EUNSUPPORTED, and msg says why
  std::string msg;
};

// threads: ctcd_set_threads (0: automatic).  streamed: the rows arrive while the kernel runs (KernelArgs::frames_ready).
// compiled(key): the build has that kernel (it is in the build's CTC_KERNEL_LIST).
template <class Compiled>
LaunchPlan plan_launch(const ctcbeam::Dims &dims, int B, int threads, int max_lds, int cu_count, const LaunchSwitches &sw, ScorerKind scorer,
                       bool streamed, const Compiled &compiled) {
  using namespace ctcbeam;
  LaunchPlan p{};
  auto refuse = [&p](std::string msg) {
    p.rc = CTCD_EUNSUPPORTED;
    p.msg = std::move(msg);
    return p;
  };
  if ((long long)dims.K * (dims.Vc_max + 2) > (1LL << 24) - 1) return refuse("beam_width * (candidates + 2) exceeds 16777215 candidate slots");
  if (dims.use_rank_table && dims.V > 32767) return refuse("vocabulary pruning with more than 32767 labels");
  const bool lm = scorer != kNoScorer, hooked = scorer == kCallbackScorer, pruned = dims.use_rank_table != 0;
  // workgroup size (measured): 1024 threads for the usual shapes; below ~1300 candidate slots 512 is marginally better
  // (fewer idle waves), fewer than that is always slower (the new-children phase wants its own waves)
  if (threads == 0) threads = (dims.S_max() <= 1300 && !lm) ? 512 : 1024;
  // a key's workgroup size: the build's own where the list has it (else 0, the run-time size); then its streamed-input twin
  auto finish = [threads, streamed, &compiled](KernelKey k) {
    k.nt = threads;
    if (!compiled(k)) k.nt = 0;
    if (streamed && ignores_streamed_input(k)) k.prof = k.prof == 3 ? 5 : 4;
    return k;
  };
  // (the LM tier has the fixed-layout kernel at 1024 threads only)
  const bool fixed = fits_fixed_layout(dims) && !sw.no_fixed_layout && (!lm || threads == 1024);
  // the second compile-time layout: the pruned default (beam <= 112, cutoff_top_n <= 40) on a vocabulary of up to 10 240 labels
  const bool fixed2 = !fixed && fits_mid_layout(dims) && !sw.no_fixed_layout && !lm && threads == 1024 && !sw.profile;
  const Dims ldims = fixed ? fixed_layout_dims(lm) : fixed2 ? mid_layout_dims() : dims;
  // two workgroups per CU (OCC2 build of the fixed-layout kernel): on request, or for batches that outnumber the CUs where the build has it
  const bool occ2 = fixed && threads == 1024 && !sw.profile && !hooked &&
                    (sw.cu_sharing == 1 || (sw.cu_sharing < 0 && B > cu_count && compiled(finish({0, 0, 1, pruned, 0, (int)scorer, 1}))));
  Work w;
  size_t far_bytes = 0;
  size_t lds = occ2 ? carve<0, true>(w, nullptr, nullptr, ldims, &far_bytes) : carve<0>(w, nullptr, nullptr, ldims, &far_bytes);
  // BIG: the HBM-scratch level of a wide beam (beam_core.h carve).  More than 65535 candidate slots (cutoff_top_n >= V with thousands
  // of labels): level 3, 32-bit slot indices and everything per slot in HBM -- the reference has no such limit (decoder_utils.cpp:33-35)
  int big = 0;
  if (dims.S_max() > 65535) {
    big = 3;
    lds = carve<3>(w, nullptr, nullptr, dims, &far_bytes);
  } else if (lds + 2048 > (size_t)max_lds) {  // wide beam: rare-path arrays go to HBM scratch
    big = 1;
    lds = carve<1>(w, nullptr, nullptr, dims, &far_bytes);
    if (lds + 2048 > (size_t)max_lds) {  // wider still: the slot keys and the rarely read per-entry arrays follow them
      big = 2;
      lds = carve<2>(w, nullptr, nullptr, dims, &far_bytes);
    }
  }
  // the first wide-beam layout at its compile-time size (LAYOUT 3: beam <= 500 over <= 29 labels, no pruning, no scorer)
  bool wide3 = false;
  if (big == 1 && fits_wide_layout(dims) && !sw.no_fixed_layout && !lm && threads == 1024 && !sw.profile) {
    size_t fb3 = 0;
    const size_t lds3 = carve<1>(w, nullptr, nullptr, wide_layout_dims(), &fb3);
    if (lds3 + 2048 <= (size_t)max_lds) { wide3 = true; lds = lds3; far_bytes = fb3; }
  }
  if (lds + 2048 > (size_t)max_lds)
    return refuse("beam_width * (candidates + 2) needs " + std::to_string(lds) + " B of LDS, more than one workgroup has");
  // (the word-model builds, LM 2, exist in the fixed layout below the HBM levels)
  const int lm_build = (scorer == kWordScorer && (big || !fixed)) ? 1 : scorer;
  KernelKey k{0, big, wide3 ? 3 : big ? 0 : fixed2 ? 2 : fixed ? 1 : 0, pruned, 0, lm_build, occ2};
  if (sw.profile) {
    k.prof = sw.tl_armed ? 2 : 1;
  } else if (fixed && !big && threads == 1024 && !lm && !occ2) {
    // chain-shaped beams (blank-dominated rows: what acoustic models emit): the build whose phase A1 searches four subtrees per wave
    KernelKey sub = k;
    sub.prof = 3;
    if (sw.subtree_mode == 1 || (sw.subtree_mode < 0 && sw.subtree_on && compiled(finish(sub)))) k.prof = 3;
  }
  p.key = finish(k);
  p.threads = threads;
  p.lds = lds;
  p.far_bytes = (far_bytes + 255) / 256 * 256;
  if (!compiled(p.key))
    return refuse("this build has no decode kernel <PROF " + std::to_string(p.key.prof) + ", BIG " + std::to_string(p.key.big) + ", LAYOUT " +
                  std::to_string(p.key.layout) + ", PRUNED " + std::to_string(p.key.pruned) + ", NT " + std::to_string(p.key.nt) + ", LM " +
                  std::to_string(p.key.lm) + ", OCC2 " + std::to_string(p.key.occ2) + "> for this call (CTC_KERNEL_LIST)");
  return p;
}

}  // namespace ctcdk
