// stream_blank_skip.h -- the blank-frame filter of blank_skip.h in front of every chunk of a live stream (include/ctcdecode_amd.h
// "Blank-frame filter of live streams").  The decision is blank_skip.h's: frame t of a chunk is SKIPPED iff t < n and v > c.  What a
// stream adds is the carry between calls: stream b has decoded frames_b frames (the kept ones) of the seen_b frames it has been fed,
// and owns a map on the device, map_b[i] = index among the seen frames of the i-th kept one.  The chunk scan writes, for the kept
// frame t of rank r inside the chunk,
//     kept[b][r] = t                      the chunk-local list ctc_blank_gather_kernel reads
//     map_b[frames_b + r] = seen_b + t    the stream's map, continued
// and n'[b], the chunk's kept count.  The decode then sees the kept rows with seq_lens = n', and every time step s a call reports
// goes back through map_b[s], guarded by (unsigned)s < frames_b.
//
// All index arithmetic lives here as CTC_HD code: the kernels of stream_blank_skip.hip and the host twin
// (tests/native/stream_blank_skip_host.cpp) compile the same routines.
#pragma once
#include "blank_skip.h"

namespace ctcsskip {

using ctcskip::kScanThreads;
using ctcskip::kScanWaves;
using ctcskip::kRemapThreads;

// One stream's entry of a call's argument table (16 bytes).  For the scan: frames / seen BEFORE the chunk.  For the remaps: frames
// = the stream's kept frames when the remap runs (the guard), seen unused.
struct StreamSkipItem {
  int32_t *map;
  int32_t frames;
  int32_t seen;
};

// ... and of the row remap's table: `rows` non-null: the item's rows start there (rows_per_item rows of row_stride words) instead
// of at their place in the call's one tensor (ctcd_stream_commit's label blocks lie one per stream)
struct StreamRemapItem {
  const int32_t *map;
  int32_t *rows;
  int32_t frames;
  int32_t pad;
};

// the rank of a kept frame inside its chunk: the kept frames of the passes before it (carry), of the waves before its own in this
// pass (below) and of the lanes before its own in its wave (before)
CTC_HD int chunk_rank(int carry, int below, int before) { return carry + below + before; }

// what the scan stores for the kept frame t of rank r of the chunk (r < n <= T; the map holds frames + n entries at least)
CTC_HD void scan_store(const StreamSkipItem &it, int32_t *kept_b, int rank, int t) {
  kept_b[rank] = t;
  it.map[(size_t)it.frames + (size_t)rank] = it.seen + t;
}

// entries a map needs before a chunk of `len` frames is scanned, and the capacity a map that lacks them grows to (doubling)
CTC_HD long long map_need(long long frames, int len) { return frames + (long long)(len < 0 ? 0 : len); }
CTC_HD long long map_grown_cap(long long cap, long long need) {
  long long c = cap < 256 ? 256 : cap;
  while (c < need) c *= 2;
  return c;
}

// ---- remap ----------------------------------------------------------------------------------------------------------------------
// a reported time step s goes back to map[s]; a word that is no index of a decoded frame is left alone (a wrong decode must not
// become an out-of-bounds read here)
CTC_HD int32_t remap_step(int32_t s, const int32_t *map, int32_t frames) { return (uint32_t)s < (uint32_t)(frames < 0 ? 0 : frames) ? map[s] : s; }
// ... and the same on a compact label record, label | frame << 16: the image must fit the 16 bits too (the compact route is taken
// only while it does; a record whose image would not is left alone)
CTC_HD uint32_t remap_record(uint32_t rec, const int32_t *map, int32_t frames) {
  const uint32_t s = rec >> 16;
  if (s >= (uint32_t)(frames < 0 ? 0 : frames)) return rec;
  const uint32_t m = (uint32_t)map[s];
  return m < 65536u ? (rec & 0xffffu) | (m << 16) : rec;
}

// the reported part of result row `row` (of rows_per_item rows per item): words [0, n) with n = its length less the item's `since`
// (ctcd_stream_peek reports a row from depth since[b] on), clamped to the row's stride
CTC_HD int row_words(const int32_t *lens, const int32_t *since, long long row, int b, long long row_stride) {
  long long n = (long long)lens[row] - (since ? (long long)since[b] : 0);
  n = n < 0 ? 0 : n;
  return (int)(n > row_stride ? row_stride : n);
}
CTC_HD int32_t *row_base(const StreamRemapItem &it, int32_t *ts, long long row, int p, long long row_stride) {
  return it.rows ? it.rows + (size_t)p * (size_t)row_stride : ts + (size_t)row * (size_t)row_stride;
}

// the compact route holds 16-bit frame numbers: it is taken only while every seen-index the call can report fits them
CTC_HD bool compact_route_ok(long long seen, int T) { return seen + (long long)(T < 0 ? 0 : T) <= 65536; }

// ---- the scan and both remaps, sequentially (the host twin; the kernels of stream_blank_skip.hip are these loops spread over a
// workgroup).  The scan walks the chunk as the device does: passes of kScanThreads frames, waves of 64, a ballot per wave. ----------
template <int DT>
inline void scan_chunk_item_host(const void *rows, const int32_t *seq_lens, const StreamSkipItem *tab, int b, int T, int V, int blank_id, float c,
                                 int32_t *kept, int32_t *kept_lens) {
  const int n = ctcskip::clamped_len(seq_lens, b, T);
  const StreamSkipItem it = tab[b];
  int32_t *kb = kept + (size_t)b * T;
  int carry = 0;
  for (int t0 = 0; t0 < n; t0 += kScanThreads) {
    int below = 0;
    for (int wave = 0; wave < kScanWaves; ++wave) {
      unsigned long long mask = 0;
      for (int lane = 0; lane < 64; ++lane) {
        const int t = t0 + wave * 64 + lane;
        if (t < n && ctcskip::frame_kept<DT>(rows, b, t, T, V, blank_id, c)) mask |= 1ull << lane;
      }
      for (int lane = 0; lane < 64; ++lane)
        if (mask >> lane & 1) scan_store(it, kb, chunk_rank(carry, below, __builtin_popcountll(mask & ((1ull << lane) - 1))), t0 + wave * 64 + lane);
      below += __builtin_popcountll(mask);
    }
    carry += below;
  }
  kept_lens[b] = carry;
}

inline void remap_rows_item_host(int32_t *ts, const int32_t *lens, const int32_t *since, const StreamRemapItem *tab, int b, int rows_per_item,
                                 long long row_stride) {
  const StreamRemapItem it = tab[b];
  for (int p = 0; p < rows_per_item; ++p) {
    const long long row = (long long)b * rows_per_item + p;
    const int n = row_words(lens, since, row, b, row_stride);
    int32_t *r = row_base(it, ts, row, p, row_stride);
    for (int i = 0; i < n; ++i) r[i] = remap_step(r[i], it.map, it.frames);
  }
}

inline void remap_compact_item_host(const int32_t *hdr, const int32_t *ent, uint32_t *labels, const StreamRemapItem *tab, int b, int K) {
  const StreamRemapItem it = tab[b];
  const int nres = ctcskip::clamp_count(hdr[(size_t)b * 4], K);
  const uint32_t first = (uint32_t)hdr[(size_t)b * 4 + 2], total = (uint32_t)hdr[(size_t)b * 4 + 1];
  for (int j = 0; j < nres; ++j) {
    const int32_t *e = ent + ((size_t)b * K + j) * 4;
    const int lcp = j == 0 ? 0 : e[1], own = e[2] - lcp;
    for (int q = 0; q < own; ++q) {
      const uint32_t at = (uint32_t)e[3] + (uint32_t)q;
      if (at - first < total) labels[at] = remap_record(labels[at], it.map, it.frames);  // (inside the item's own labels)
    }
  }
}

// ---- what stream_blank_skip.hip exports to the library's host file (ctcdecode_amd.hip); every launcher returns a hipError_t as int --
// the chunk scan: rows [B, T, V] of element type `dtype` (CTCD_DTYPE_*), seq_lens [B] and tab [B] readable by the device; writes
// kept [B, T] (entries [0, n') of each row), kept_lens [B] and the streams' maps
int launch_chunk_scan(const void *rows, const int32_t *seq_lens, const StreamSkipItem *tab, int B, int T, int V, int blank_id, float c, int dtype,
                      int32_t *kept, int32_t *kept_lens, void *stream);
// the row remap: n_rows = B * rows_per_item rows; lens [n_rows], since [B] or null, tab [B]
int launch_remap_rows(int32_t *ts, const int32_t *lens, const int32_t *since, const StreamRemapItem *tab, int B, int rows_per_item, long long row_stride,
                      void *stream);
// ... and the compact one
int launch_remap_compact(const int32_t *hdr, const int32_t *ent, uint32_t *labels, const StreamRemapItem *tab, int B, int K, void *stream);

}  // namespace ctcsskip

namespace ctcskip {
// blank_skip.hip: ctc_blank_gather_kernel on a chunk (the word size chosen as ctcd_blank_skip chooses it); a hipError_t as int
int launch_blank_gather(const void *in, void *out, const int32_t *kept, const int32_t *kept_lens, int B, int T, int V, int dtype, void *stream);
}  // namespace ctcskip
