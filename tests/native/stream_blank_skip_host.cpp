// Host twin of the blank-frame filter of live streams (ctcdecode_amd/csrc/stream_blank_skip.h): the header's scan with carry -- passes
// of 1024 frames, waves of 64, ranks from a ballot -- and both remaps behind a C ABI, run sequentially.  A "stream" here is the triple
// the library keeps per stream: frames decoded, frames seen, the map.  Test infrastructure only.
#include "../../ctcdecode_amd/csrc/stream_blank_skip.h"

#include <vector>

// One chunk call on B streams.  dtype: 0 float32, 1 float16, 2 bfloat16.  rows [B, T, V]; seq_lens [B] or NULL; maps[b] has room for
// frames[b] + T entries.  Writes kept [B, T] (entries [0, n') of each row alone), kept_lens [B] and maps[b][frames[b] ...), and -- the
// launch was accepted -- advances frames[b] / seen[b].  Returns 0, or -1 for bad arguments.
extern "C" int ctcsskip_host_chunk(const void *rows, int dtype, const int32_t *seq_lens, int B, int T, int V, int blank_id, float c, int32_t *const *maps,
                                   long long *frames, long long *seen, int32_t *kept, int32_t *kept_lens) {
  namespace ss = ctcsskip;
  namespace cs = ctcskip;
  if (!rows || !maps || !frames || !seen || !kept || !kept_lens || B <= 0 || T <= 0 || V <= 0 || blank_id < 0 || blank_id >= V || dtype < 0 || dtype > 2) return -1;
  std::vector<ss::StreamSkipItem> tab((size_t)B);
  for (int b = 0; b < B; ++b) tab[b] = ss::StreamSkipItem{maps[b], (int32_t)frames[b], (int32_t)seen[b]};
  for (int b = 0; b < B; ++b) {
    if (dtype == cs::kSkipF16) ss::scan_chunk_item_host<cs::kSkipF16>(rows, seq_lens, tab.data(), b, T, V, blank_id, c, kept, kept_lens);
    else if (dtype == cs::kSkipBF16) ss::scan_chunk_item_host<cs::kSkipBF16>(rows, seq_lens, tab.data(), b, T, V, blank_id, c, kept, kept_lens);
    else ss::scan_chunk_item_host<cs::kSkipF32>(rows, seq_lens, tab.data(), b, T, V, blank_id, c, kept, kept_lens);
  }
  for (int b = 0; b < B; ++b) {
    frames[b] += kept_lens[b];
    seen[b] += cs::clamped_len(seq_lens, b, T);
  }
  return 0;
}

// The row remap: ts [B, rows_per_item, row_stride] (or, where rows[b] is non-NULL, the item's rows start there), lens [B * rows_per_item],
// since [B] or NULL, maps / frames [B].
extern "C" void ctcsskip_host_remap_rows(int32_t *ts, int32_t *const *rows, const int32_t *lens, const int32_t *since, const int32_t *const *maps,
                                         const int32_t *frames, int B, int rows_per_item, long long row_stride) {
  std::vector<ctcsskip::StreamRemapItem> tab((size_t)B);
  for (int b = 0; b < B; ++b) tab[b] = ctcsskip::StreamRemapItem{maps[b], rows ? rows[b] : nullptr, frames[b], 0};
  for (int b = 0; b < B; ++b) ctcsskip::remap_rows_item_host(ts, lens, since, tab.data(), b, rows_per_item, row_stride);
}

extern "C" void ctcsskip_host_remap_compact(const int32_t *hdr, const int32_t *ent, uint32_t *labels, const int32_t *const *maps, const int32_t *frames, int B,
                                            int K) {
  std::vector<ctcsskip::StreamRemapItem> tab((size_t)B);
  for (int b = 0; b < B; ++b) tab[b] = ctcsskip::StreamRemapItem{maps[b], nullptr, frames[b], 0};
  for (int b = 0; b < B; ++b) ctcsskip::remap_compact_item_host(hdr, ent, labels, tab.data(), b, K);
}

extern "C" long long ctcsskip_host_map_grown_cap(long long cap, long long need) { return ctcsskip::map_grown_cap(cap, need); }
extern "C" int ctcsskip_host_compact_route_ok(long long seen, int T) { return ctcsskip::compact_route_ok(seen, T) ? 1 : 0; }
