// Host twin of the blank-frame filter (ctcdecode_amd/csrc/blank_skip.h): the header's per-frame decision, rank bookkeeping, tile walk
// of the gather and both remaps behind a C ABI, run sequentially.  Test infrastructure only.
#include "../../ctcdecode_amd/csrc/blank_skip.h"

namespace {
struct alignas(16) W16 { uint32_t w[4]; };  // the 16-byte word of the gather's fast path
}

// dtype: 0 float32, 1 float16, 2 bfloat16 (ctcd_set_input_dtype).  out_rows: rows [b][0, out_lens[b]) are written, nothing else.
// Returns the word size the gather used (16, 4 or 2), or -1 for bad arguments.
extern "C" int ctcskip_host_filter(const void *x, int dtype, const int32_t *seq_lens, int B, int T, int V, int blank_id, float c, void *out_rows,
                                   int32_t *out_lens, int32_t *out_kept) {
  namespace cs = ctcskip;
  if (!x || !out_rows || !out_lens || !out_kept || B <= 0 || T <= 0 || V <= 0 || blank_id < 0 || blank_id >= V || dtype < 0 || dtype > 2) return -1;
  for (int b = 0; b < B; ++b) {
    if (dtype == cs::kSkipF16) cs::scan_item_host<cs::kSkipF16>(x, seq_lens, b, T, V, blank_id, c, out_kept, out_lens);
    else if (dtype == cs::kSkipBF16) cs::scan_item_host<cs::kSkipBF16>(x, seq_lens, b, T, V, blank_id, c, out_kept, out_lens);
    else cs::scan_item_host<cs::kSkipF32>(x, seq_lens, b, T, V, blank_id, c, out_kept, out_lens);
  }
  const size_t eb = cs::elem_bytes(dtype), row_bytes = (size_t)V * eb;
  const bool v16 = cs::gather_vec16(row_bytes, (uintptr_t)x, (uintptr_t)out_rows);
  for (int b = 0; b < B; ++b) {
    if (v16) cs::gather_item_host<W16>(x, b, T, row_bytes, out_kept, out_lens, out_rows);
    else if (eb == 4) cs::gather_item_host<uint32_t>(x, b, T, row_bytes, out_kept, out_lens, out_rows);
    else cs::gather_item_host<uint16_t>(x, b, T, row_bytes, out_kept, out_lens, out_rows);
  }
  return v16 ? 16 : (int)eb;
}

extern "C" void ctcskip_host_remap_timesteps(int32_t *timesteps, const int32_t *out_lens, const int32_t *kept, const int32_t *kept_lens, int B, int K, int T) {
  for (int b = 0; b < B; ++b) ctcskip::remap_timesteps_item_host(timesteps, out_lens, kept, kept_lens, b, K, T);
}

extern "C" void ctcskip_host_remap_compact(const int32_t *hdr, const int32_t *ent, uint32_t *labels, const int32_t *kept, const int32_t *kept_lens, int B, int K,
                                           int T) {
  for (int b = 0; b < B; ++b) ctcskip::remap_compact_item_host(hdr, ent, labels, kept, kept_lens, b, K, T);
}

// the widening of one half element (dtype 1 / 2), as float32 bits
extern "C" uint32_t ctcskip_host_widen_bits(int dtype, uint16_t u) {
  const float f = dtype == ctcskip::kSkipF16 ? ctcskip::widen_at<ctcskip::kSkipF16>(&u, 0) : ctcskip::widen_at<ctcskip::kSkipBF16>(&u, 0);
  uint32_t r;
  memcpy(&r, &f, 4);
  return r;
}

extern "C" int ctcskip_host_tile_rows(long long row_bytes) { return ctcskip::gather_tile_rows((size_t)row_bytes); }
extern "C" int ctcskip_host_tiles(int T, int tile_rows) { return ctcskip::gather_tiles(T, tile_rows); }
