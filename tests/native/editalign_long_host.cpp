// Host twin of the long edit alignments (ctcdecode_amd/csrc/editlong.h, long_align_host) behind a C ABI.  The slot is a host buffer of
// exactly long_align_slot_bytes of the pair's two lengths, so that a checkpoint or a direction word outside it is a sanitizer report.
// -DEDITALIGN_LONG_MAIN: a program of its own, meant for -fsanitize=address,undefined.  Every argument is a case file, int32
// {lx, ly, W}, x, y and the maps the reference expects; prints "<checks> checks, <n> failures".  Test infrastructure only.
#include <cstdio>
#include <vector>

#include "../../ctcdecode_amd/csrc/editlong.h"

using namespace ctcedit;

// One pair of rows, both beyond 0 tokens: the maps, written in full; out = (H, S, Del, I), the blocks swept again, the slot's bytes.
extern "C" void ctcedit_align_long_host_pair(const int32_t *x, int lx, const int32_t *y, int ly, int W, int32_t *x_to_y, int32_t *y_to_x, int32_t *out) {
  const bool x_strip = lx <= ly;
  const size_t bytes = long_align_slot_bytes(lx, ly);
  std::vector<long long> ring((size_t)W * kLongRing, -1);
  std::vector<KeyLane64> lanes((size_t)W * kEditLanes);
  std::vector<char> slot(bytes, (char)0xA5);
  for (int p = 0; p < lx; ++p) x_to_y[p] = -1;
  for (int p = 0; p < ly; ++p) y_to_x[p] = -1;
  const long long key = long_align_host(x_strip ? x : y, x_strip ? lx : ly, x_strip ? y : x, x_strip ? ly : lx, W, x_strip, ring.data(), slot.data(), lx, ly, lanes.data(), x_to_y, y_to_x, &out[4]);
  CountCell::result(key, lx, ly, out, nullptr);
  out[5] = (int32_t)bytes;
}

#ifdef EDITALIGN_LONG_MAIN
int main(int argc, char **argv) {
  int failures = 0;
  for (int i = 1; i < argc; ++i) {
    std::FILE *f = std::fopen(argv[i], "rb");
    int32_t h[3], out[6];
    if (!f || std::fread(h, 4, 3, f) != 3) return 2;
    const size_t lx = (size_t)h[0], ly = (size_t)h[1];
    std::vector<int32_t> x(lx), y(ly), want_x(lx), want_y(ly), xm(lx), ym(ly);
    if (std::fread(x.data(), 4, lx, f) != lx || std::fread(y.data(), 4, ly, f) != ly || std::fread(want_x.data(), 4, lx, f) != lx || std::fread(want_y.data(), 4, ly, f) != ly) return 2;
    std::fclose(f);
    ctcedit_align_long_host_pair(x.data(), (int)lx, y.data(), (int)ly, h[2], xm.data(), ym.data(), out);
    if (xm != want_x || ym != want_y) failures += std::printf("FAIL %s (%d x %d, %d waves)\n", argv[i], h[0], h[1], h[2]) > 0;
  }
  std::printf("%d checks, %d failures\n", argc - 1, failures);
  return failures ? 1 : 0;
}
#endif
