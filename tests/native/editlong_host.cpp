// Host twin of the long edit pairs (ctcdecode_amd/csrc/editlong.h): the sequential routine at the end of that header and the schedule
// functions, behind a C ABI.  The rings and the slot are host buffers of exactly the sizes the device uses.  Test infrastructure only.
#include <cstdlib>
#include <vector>

#include "../../ctcdecode_amd/csrc/editlong.h"

using namespace ctcedit;

template <class P> static void pair(const int32_t *x, int lx, const int32_t *y, int ly, int W, int32_t *out) {
  typedef typename P::V V;
  const bool x_strip = lx <= ly;
  std::vector<V> ring((size_t)W * kLongRing, (V)-1);
  V *col = (V *)std::malloc(long_slot_bytes(lx, ly, P::kCounts));  // exactly the slot: an access outside it is a sanitizer report
  std::vector<typename P::L> lanes((size_t)W * kEditLanes);
  const V v = long_pair_host<P>(x_strip ? x : y, x_strip ? lx : ly, x_strip ? y : x, x_strip ? ly : lx, W, ring.data(), col, lanes.data());
  std::free(col);
  P::result(v, lx, ly, out, nullptr);
}
// one pair of non-empty rows: out[0] = the distance, or out[0..4) = (H, S, Del, I)
extern "C" void ctcedit_long_host_pair(const int32_t *x, int lx, const int32_t *y, int ly, int W, int counts, int32_t *out) {
  if (counts) pair<CountCell>(x, lx, y, ly, W, out);
  else pair<DistCell>(x, lx, y, ly, W, out);
}
// the schedule: out = {active, tile, block of wave w in global block g | global blocks, blocks of a tile | of a tile's block q: the first
// row read, the rows done after it, the row lane 63 completes at its first step | the ring index of row q | a distance's slot, bytes}
extern "C" void ctcedit_long_host_sched(int g, int w, int m, int n, int W, int q, int32_t *out) {
  const LongSlot s = long_slot(g, w, m, n, W);
  out[0] = s.active, out[1] = s.tile, out[2] = s.block, out[3] = (int)long_blocks(m, n, W), out[4] = long_tile_blocks(m);
  out[5] = long_row_first(q), out[6] = long_rows_done(q, m), out[7] = long_edge_row(q * kLongBlock), out[8] = long_ring_index(q);
  out[9] = (int)long_slot_bytes(m, n, false);
}
