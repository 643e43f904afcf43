// keyword_long.h -- the shapes of the long keyword kernel (keyword_long.hip; include/ctcdecode_amd.h "Keyword search",
// ctcd_set_long_keywords): keywords of 65 .. 2048 labels, eight labels per lane.  The definition, the cell rules and the validation are
// keyword.h's and are used as they are; what is here is the arithmetic of the launch only, CTC_HD so that a host program can read it.
//
// A lane holds eight consecutive labels, a wave 512.  A keyword takes 1, 2 or 4 waves (its class, by L_stride); the workgroup stays four
// waves, so it holds 4, 2 or 1 keywords.  The waves of a keyword walk the item's frames one step of frames behind each other.
#pragma once
#include "keyword.h"

namespace ctckw {

constexpr int kKwLongMaxLabels = 2048;                      // four waves of 512 labels
constexpr int kKwLongPerLane = 8;                           // labels per lane: 16 (value, start) pairs in registers
constexpr int kKwLongPerWave = 64 * kKwLongPerLane;         // 512
constexpr int kKwLongWaves = kKwThreads / 64;               // the waves of a workgroup
constexpr int kKwLongGatherStep = 4;                        // frames per step on the gathered route
constexpr int kKwLongMaxStep = 32;                          // the longest step of any class and route
constexpr int kKwLongRing = 2 * kKwLongMaxStep;             // entries of a boundary's ring (used: two steps)

// the waves a keyword occupies: 1 up to 512 labels, 2 up to 1024, 4 up to 2048
CTC_HD int kwl_waves(int L_stride) { return L_stride <= kKwLongPerWave ? 1 : (L_stride <= 2 * kKwLongPerWave ? 2 : 4); }
CTC_HD int kwl_per_workgroup(int waves) { return kKwLongWaves / waves; }
// the frames of a step: what a wave walks between two barriers, and what is staged or gathered at a time
CTC_HD int kwl_step(int waves, bool staged) { return staged ? (waves == 1 ? 32 : 16) : kKwLongGatherStep; }
// the step buffers of the staged ring: a step lives until the keyword's last wave has walked it, and one is being filled
CTC_HD int kwl_staged_bufs(int waves) { return waves + 1; }
// dynamic LDS.  STAGED: the ring of step buffers of r(t, c), 32 / 24 / 40 KiB at V = 128 for 1 / 2 / 4 waves.  Gathered: a private
// region per wave of the workgroup, kKwLongGatherStep frames of its 512 positions: 32 KiB for every class.
CTC_HD size_t kwl_lds_bytes(int V, int waves) {
  return kw_staged(V) ? (size_t)kwl_staged_bufs(waves) * kwl_step(waves, true) * (size_t)V * sizeof(float)
                      : (size_t)kKwLongWaves * kKwLongGatherStep * kKwLongPerWave * sizeof(float);
}
// what ctcd_last_keyword_kernel reports: keyword.h's bits 8..11 over 128 + waves (no lane-group width is 129, 130 or 132)
CTC_HD int kwl_kernel_code(int dt, bool prob, bool staged, int waves) { return ((dt | (prob ? 4 : 0) | (staged ? 8 : 0)) << 8) | (128 + waves); }

// keyword_long.hip: the launch behind ctcd_ctc_keywords' argmax pass (dt: a ctcskip element type).  Returns the kernel's code.
int launch_keyword_long(int dt, bool prob, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank, const FrameRec *rec, const int32_t *keywords,
                        const int32_t *keyword_lens, int Q, int L_stride, float *out_sc, int32_t *out_st, int32_t *out_en, float *out_tr_v, int32_t *out_tr_s,
                        int32_t *status, void *stream);
// ctcdecode_amd.hip: what ctcd_set_long_keywords set
bool keyword_long_on(const ctcd_decoder *d);

}  // namespace ctckw
