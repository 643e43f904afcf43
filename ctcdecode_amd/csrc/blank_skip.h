// blank_skip.h -- the blank-frame filter in front of a one-shot decode (include/ctcdecode_amd.h ctcd_blank_skip): frame t of
// utterance b is SKIPPED iff t < n (n = seq_lens[b] clamped to [0, T]) and v > c, v the float32 value of the blank's entry of that
// frame (a half-precision entry widened exactly) and c a float32 the caller computed once.  The compare is an ordered, strict `>`:
// NaN is kept, a value equal to c is kept.  Kept frames keep their order: kept[b][i] = original index of the i-th kept frame,
// n'[b] their count, kept[b][n'[b]:T] = 0.  The decode then sees the kept rows with seq_lens = n', and every reported time step s
// goes back to kept[b][s].
//
// The per-frame decision and every piece of index arithmetic live here as CTC_HD code: the kernels of blank_skip.hip and the host
// twin (tests/native/blank_skip_host.cpp) compile the same routines.  No floating-point arithmetic: a widening and one compare.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef CTC_HD
#if defined(__HIPCC__)
#define CTC_HD __host__ __device__ __forceinline__
#else
#define CTC_HD inline
#endif
#endif

namespace ctcskip {

enum : int { kSkipF32 = 0, kSkipF16 = 1, kSkipBF16 = 2 };  // include/ctcdecode_amd.h CTCD_DTYPE_*

constexpr int kScanThreads = 1024;       // frames of a scan chunk = threads of the scan's workgroup (16 waves of 64)
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kGatherThreads = 256;
constexpr int kGatherTileBytes = 32768;  // kept rows of one gather workgroup: as many as fit this, at least one
constexpr int kRemapThreads = 256;       // padded results: one wave per result row; compact results: one workgroup per item

CTC_HD float bits_to_f32(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// IEEE binary16 -> binary32, exact, in integer arithmetic (subnormals, infinities and NaN payloads included)
CTC_HD uint32_t f16_to_f32_bits(uint16_t h) {
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16;
  uint32_t e = ((uint32_t)h >> 10) & 31u, m = (uint32_t)h & 0x3ffu;
  if (e == 31u) return sign | 0x7f800000u | (m << 13);
  if (e == 0u) {
    if (m == 0u) return sign;
    e = 1u;
    while (!(m & 0x400u)) { m <<= 1; --e; }  // (at most ten steps; e wraps below zero as an unsigned and is added to 112 below)
    m &= 0x3ffu;
  }
  return sign | ((e + 112u) << 23) | (m << 13);
}

// element `i` of rows of dtype DT as the float32 the decoder computes on
template <int DT> CTC_HD float widen_at(const void *rows, size_t i) {
  if (DT == kSkipF32) return ((const float *)rows)[i];
  const uint16_t u = ((const uint16_t *)rows)[i];
  return bits_to_f32(DT == kSkipBF16 ? (uint32_t)u << 16 : f16_to_f32_bits(u));
}

CTC_HD size_t elem_bytes(int dt) { return dt == kSkipF32 ? 4 : 2; }

// the definition: skipped iff v > c (ordered: false for NaN on either side)
CTC_HD bool frame_skipped(float v, float c) { return v > c; }

// an utterance's length as the decode kernels clamp it (binding.cpp:64-65)
CTC_HD int clamped_len(const int32_t *lens, int b, int T) {
  const int l = lens ? lens[b] : T;
  return l < 0 ? 0 : (l > T ? T : l);
}

// frame t of utterance b: is it kept?  (t < n is the caller's business: frames at or beyond n are never looked at)
template <int DT> CTC_HD bool frame_kept(const void *rows, int b, int t, int T, int V, int blank_id, float c) {
  return !frame_skipped(widen_at<DT>(rows, ((size_t)b * T + t) * V + blank_id), c);
}

CTC_HD int clamp_count(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- gather ---------------------------------------------------------------------------------------------------------------------
// rows of one tile, and the tiles that cover T rows (the grid is cut for the worst case, n' = T)
CTC_HD int gather_tile_rows(size_t row_bytes) {
  const size_t r = (size_t)kGatherTileBytes / (row_bytes ? row_bytes : 1);
  return r < 1 ? 1 : (int)r;
}
CTC_HD int gather_tiles(int T, int tile_rows) { return (T + tile_rows - 1) / tile_rows; }
// the 16-byte path: whole rows of 16-byte words on both sides
CTC_HD bool gather_vec16(size_t row_bytes, uintptr_t in, uintptr_t out) { return row_bytes % 16 == 0 && in % 16 == 0 && out % 16 == 0; }

// One tile of the gather -- tile `tile` of utterance b: kept rows [i0, i0 + rows), consecutive in the output.  Word w of the tile comes
// from row kept[i0 + w / row_words], word w % row_words of it; W = the copy's word (16 bytes, or the element).  The caller's share of
// the words is first, first + step, ...: a thread of the workgroup on the device, everything (0, 1) on the host.  `store(dst, value)`.
template <typename W, typename Store>
CTC_HD void gather_tile(const W *in, W *out, const int32_t *kept, const int32_t *kept_lens, int b, int tile, int T, unsigned row_words, int tile_rows,
                        unsigned first, unsigned step, Store store) {
  const int nk = clamp_count(kept_lens[b], T);
  const int i0 = tile * tile_rows;
  if (i0 >= nk) return;  // (the grid is cut for n' = T: tiles at or beyond n' leave at once)
  const int rows = nk - i0 < tile_rows ? nk - i0 : tile_rows;
  const int32_t *kb = kept + (size_t)b * T + i0;
  const W *src = in + (size_t)b * T * row_words;
  W *dst = out + ((size_t)b * T + i0) * row_words;
  const unsigned words = (unsigned)rows * row_words;  // (at most kGatherTileBytes / sizeof(W), or one row's)
  for (unsigned w = first; w < words; w += step) {
    const unsigned r = w / row_words, col = w - r * row_words;
    const int t = kb[r];
    if ((unsigned)t >= (unsigned)T) continue;  // (never for a map the scan wrote)
    store(dst + w, src[(size_t)t * row_words + col]);
  }
}

// ---- remap ----------------------------------------------------------------------------------------------------------------------
// a reported time step s of utterance b goes back to kept[s]; a word that is no index of a kept frame is left alone (a wrong
// decode must not become an out-of-bounds read here)
CTC_HD int32_t remap_step(int32_t s, const int32_t *kept_b, int n_kept) { return (unsigned)s < (unsigned)n_kept ? kept_b[s] : s; }
// ... and the same on a compact label record: label | frame << 16
CTC_HD uint32_t remap_record(uint32_t rec, const int32_t *kept_b, int n_kept) {
  const uint32_t s = rec >> 16;
  return s < (uint32_t)(n_kept < 0 ? 0 : n_kept) ? (rec & 0xffffu) | ((uint32_t)kept_b[s] << 16) : rec;
}

// ---- the whole filter and both remaps, sequentially (the host twin; the kernels of blank_skip.hip are these loops spread over a
// workgroup) -----------------------------------------------------------------------------------------------------------------------
template <int DT> inline void scan_item_host(const void *rows, const int32_t *seq_lens, int b, int T, int V, int blank_id, float c, int32_t *kept,
                                             int32_t *kept_lens) {
  const int n = clamped_len(seq_lens, b, T);
  int32_t *kb = kept + (size_t)b * T;
  int cnt = 0;
  for (int t = 0; t < n; ++t)
    if (frame_kept<DT>(rows, b, t, T, V, blank_id, c)) kb[cnt++] = t;
  kept_lens[b] = cnt;
  for (int i = cnt; i < T; ++i) kb[i] = 0;
}

// kept rows of utterance b -> out rows [0, n'), tile by tile as the device walks them; rows at or beyond n' are not written
template <typename W> inline void gather_item_host(const void *rows, int b, int T, size_t row_bytes, const int32_t *kept, const int32_t *kept_lens, void *out) {
  const int tile_rows = gather_tile_rows(row_bytes), tiles = gather_tiles(T, tile_rows);
  for (int tile = 0; tile < tiles; ++tile)
    gather_tile<W>((const W *)rows, (W *)out, kept, kept_lens, b, tile, T, (unsigned)(row_bytes / sizeof(W)), tile_rows, 0u, 1u, [](W *d, const W &v) { *d = v; });
}

inline void remap_timesteps_item_host(int32_t *timesteps, const int32_t *out_lens, const int32_t *kept, const int32_t *kept_lens, int b, int K, int T) {
  const int nk = clamp_count(kept_lens[b], T);
  // (the scan's map is strictly increasing: its last entry is nk - 1 exactly when no frame of the utterance was skipped, and then
  //  every time step is its own image -- the item's rows are not touched)
  if (nk == 0 || kept[(size_t)b * T + nk - 1] == nk - 1) return;
  for (int p = 0; p < K; ++p) {
    const int L = clamp_count(out_lens[(size_t)b * K + p], T);
    int32_t *row = timesteps + ((size_t)b * K + p) * T;
    for (int i = 0; i < L; ++i) row[i] = remap_step(row[i], kept + (size_t)b * T, nk);
  }
}

inline void remap_compact_item_host(const int32_t *hdr, const int32_t *ent, uint32_t *labels, const int32_t *kept, const int32_t *kept_lens, int b,
                                    int K, int T) {
  const int nk = clamp_count(kept_lens[b], T);
  const int nres = clamp_count(hdr[(size_t)b * 4], K);
  const uint32_t first = (uint32_t)hdr[(size_t)b * 4 + 2], total = (uint32_t)hdr[(size_t)b * 4 + 1];
  for (int j = 0; j < nres; ++j) {
    const int32_t *e = ent + ((size_t)b * K + j) * 4;
    const int lcp = j == 0 ? 0 : e[1], own = e[2] - lcp;
    for (int q = 0; q < own; ++q) {
      const uint32_t at = (uint32_t)e[3] + (uint32_t)q;
      if (at - first < total) labels[at] = remap_record(labels[at], kept + (size_t)b * T, nk);  // (inside the item's own labels)
    }
  }
}

// ---- what blank_skip.hip exports to the library's host file, and what that file lends it (ctcdecode_amd.hip) ---------------------
struct SkipDecoderInfo {
  int device;
  int in_dtype;
};

}  // namespace ctcskip

struct ctcd_decoder;
namespace ctcskip {
int skip_decoder_info(const ctcd_decoder *d, SkipDecoderInfo *out);  // ctcdecode_amd.hip: the decoder's device and ctcd_set_input_dtype
int skip_fail(int code, const char *msg);                             // ctcdecode_amd.hip: sets ctcd_last_error, returns code
}  // namespace ctcskip
