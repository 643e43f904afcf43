// Stand-alone driver of the blank-frame filter's host twin (blank_skip_host.cpp), for a sanitizer build on the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/native/blank_skip_host_main.cpp -o blank_skip_host_main && ./blank_skip_host_main
// Seeded batches of every dtype, row alignment and length pattern go through the filter and both remaps in exactly-sized heap
// buffers, and are compared with loops written here from the definition alone; words the definition does not name (rows at or
// beyond n', result words beyond a valid prefix, label records outside an item's range) must keep their sentinels.
// Test infrastructure only.
#include "blank_skip_host.cpp"

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

namespace {

int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (++g_fail < 20) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

// float32 -> the half formats, round to nearest even (the inputs of the driver; the code under test only widens)
uint16_t to_bf16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
uint16_t to_f16(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u;
  u &= 0x7fffffffu;
  if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
  if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to 65536 or beyond
  if (u < 0x38800000u) {                                     // below 2^-14: a multiple of 2^-24
    float a;
    memcpy(&a, &u, 4);
    return (uint16_t)(sign | (uint32_t)std::nearbyint(a * 16777216.0f));
  }
  uint32_t h = (((u >> 23) - 112u) << 10) | ((u & 0x7fffffu) >> 13);
  const uint32_t rem = u & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;
  return (uint16_t)(sign | h);
}
// the value of a half element by the formats' definitions (ldexp), independent of the header under test
float from_half(int dtype, uint16_t u) {
  if (dtype == 2) { const uint32_t w = (uint32_t)u << 16; float f; memcpy(&f, &w, 4); return f; }
  const int e = (u >> 10) & 31, m = u & 0x3ff;
  const float a = e == 31 ? (m ? NAN : INFINITY) : e == 0 ? std::ldexp((float)m, -24) : std::ldexp((float)(1024 + m), e - 25);
  return (u & 0x8000) ? -a : a;
}

void widen_all() {  // every binary16 / bfloat16 pattern against the formats' definitions, bit for bit
  for (int dtype = 1; dtype <= 2; ++dtype)
    for (uint32_t u = 0; u < 65536u; ++u) {
      const float want = from_half(dtype, (uint16_t)u);
      uint32_t wb;
      memcpy(&wb, &want, 4);
      const uint32_t got = ctcskip_host_widen_bits(dtype, (uint16_t)u);
      if (std::isnan(want)) EXPECT((got & 0x7f800000u) == 0x7f800000u && (got & 0x7fffffu), "dtype %d 0x%04x: NaN lost", dtype, u);
      else EXPECT(got == wb, "dtype %d 0x%04x: 0x%08x want 0x%08x", dtype, u, got, wb);
    }
}

void one_case(unsigned seed, int dtype, int B, int T, int V, int blank_id, float c, int len_mode) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> ud(-6.f, 0.f);
  const size_t eb = dtype ? 2 : 4, n = (size_t)B * T * V;
  std::vector<unsigned char> x(n * eb), out(n * eb, 0xA5);
  std::vector<float> blank((size_t)B * T);
  for (size_t i = 0; i < n; ++i) {
    float v = ud(rng);
    if (i % V == (size_t)blank_id) {
      const unsigned k = rng() % 16;
      if (k == 0) v = c;  // exactly the bound: kept
      else if (k == 1) v = NAN;
      else if (k == 2) v = INFINITY;
      else if (k == 3) v = -INFINITY;
      else if (k < 10) v = c + 0.5f;
    }
    if (dtype == 0) memcpy(&x[i * 4], &v, 4);
    else { const uint16_t h = dtype == 1 ? to_f16(v) : to_bf16(v); memcpy(&x[i * 2], &h, 2); v = from_half(dtype, h); }
    if (i % V == (size_t)blank_id) blank[i / V] = v;
  }
  std::vector<int32_t> lens(B);
  for (int b = 0; b < B; ++b)
    lens[b] = len_mode == 0 ? T : len_mode == 1 ? (int)(rng() % (T + 1)) : (b % 3 == 0 ? 0 : b % 3 == 1 ? T + 5 : -3);
  std::vector<int32_t> kept((size_t)B * T, -77), klen(B, -77);
  const int word = ctcskip_host_filter(x.data(), dtype, len_mode == 0 && (seed & 1) ? nullptr : lens.data(), B, T, V, blank_id, c, out.data(), klen.data(), kept.data());
  EXPECT(word == (((size_t)V * eb) % 16 == 0 ? 16 : (int)eb), "word size %d for V %d dtype %d", word, V, dtype);
  for (int b = 0; b < B; ++b) {
    const int nb = lens[b] < 0 ? 0 : lens[b] > T ? T : lens[b];
    std::vector<int> want;
    for (int t = 0; t < nb; ++t)
      if (!(blank[(size_t)b * T + t] > c)) want.push_back(t);
    EXPECT(klen[b] == (int)want.size(), "item %d: %d kept, want %zu", b, klen[b], want.size());
    if (klen[b] != (int)want.size()) continue;
    for (int i = 0; i < T; ++i) {
      const int w = i < (int)want.size() ? want[i] : 0;
      EXPECT(kept[(size_t)b * T + i] == w, "item %d kept[%d] = %d want %d", b, i, kept[(size_t)b * T + i], w);
    }
    const size_t rb = (size_t)V * eb;
    for (int i = 0; i < T; ++i) {
      const unsigned char *o = &out[((size_t)b * T + i) * rb];
      if (i < (int)want.size()) EXPECT(memcmp(o, &x[((size_t)b * T + want[i]) * rb], rb) == 0, "item %d row %d differs", b, i);
      else for (size_t k = 0; k < rb; ++k) EXPECT(o[k] == 0xA5, "item %d row %d beyond n' was written", b, i);
    }
  }
  // remap of padded results: valid prefixes hold indices below n', one word out of range; the rest holds sentinels
  const int K = 3;
  std::vector<int32_t> ts((size_t)B * K * T), want_ts, ol((size_t)B * K);
  for (int b = 0; b < B; ++b)
    for (int p = 0; p < K; ++p) {
      const int L = klen[b] > 0 ? (int)(rng() % (klen[b] + 1)) : 0;
      ol[(size_t)b * K + p] = p == 2 ? -1 : L;
      for (int i = 0; i < T; ++i) ts[((size_t)b * K + p) * T + i] = i < L && klen[b] > 0 ? (int)(rng() % klen[b]) : 1000000 + i;
      if (L > 1) ts[((size_t)b * K + p) * T + 1] = (rng() & 1) ? -5 : klen[b];  // no kept frame's index: left alone
    }
  want_ts = ts;
  for (int b = 0; b < B; ++b)
    for (int p = 0; p < K; ++p)
      for (int i = 0; i < ol[(size_t)b * K + p]; ++i) {
        int32_t &w = want_ts[((size_t)b * K + p) * T + i];
        if (w >= 0 && w < klen[b]) w = kept[(size_t)b * T + w];
      }
  ctcskip_host_remap_timesteps(ts.data(), ol.data(), kept.data(), klen.data(), B, K, T);
  EXPECT(ts == want_ts, "remap of the padded results differs (seed %u)", seed);
  // remap of compact results: per item two entries, the second sharing one label with the first; a gap of foreign records between items
  std::vector<int32_t> hdr((size_t)B * 4), ent((size_t)B * K * 4, 0);
  std::vector<uint32_t> lab, want_lab;
  for (int b = 0; b < B; ++b) {
    lab.push_back(0xFFFF0000u | 7u);  // foreign record in front of the item: untouched
    const int d0 = klen[b] > 2 ? 2 : klen[b], d1 = klen[b] > 2 ? 3 : d0;
    hdr[(size_t)b * 4] = klen[b] > 0 ? 2 : 1; hdr[(size_t)b * 4 + 2] = (int32_t)lab.size();
    int32_t *e0 = &ent[((size_t)b * K) * 4], *e1 = e0 + 4;
    e0[0] = 0; e0[1] = 12345; e0[2] = d0; e0[3] = (int32_t)lab.size();  // (entry 0's shared count is not read)
    for (int q = 0; q < d0; ++q) lab.push_back((uint32_t)(rng() % 29) | ((uint32_t)(rng() % klen[b]) << 16));
    const int shared = d0 > 0 ? 1 : 0;
    e1[0] = 1; e1[1] = shared; e1[2] = d1; e1[3] = (int32_t)lab.size();
    for (int q = shared; q < d1; ++q) lab.push_back((uint32_t)(rng() % 29) | ((uint32_t)(rng() % klen[b]) << 16));
    hdr[(size_t)b * 4 + 1] = (int32_t)lab.size() - hdr[(size_t)b * 4 + 2];
  }
  want_lab = lab;
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < hdr[(size_t)b * 4 + 1]; ++i) {
      uint32_t &r = want_lab[(size_t)hdr[(size_t)b * 4 + 2] + i];
      r = (r & 0xffffu) | ((uint32_t)kept[(size_t)b * T + (r >> 16)] << 16);
    }
  ctcskip_host_remap_compact(hdr.data(), ent.data(), lab.data(), kept.data(), klen.data(), B, K, T);
  EXPECT(lab == want_lab, "remap of the compact results differs (seed %u)", seed);
}

}  // namespace

int main() {
  widen_all();
  unsigned seed = 1, cases = 0;
  const int Vs[] = {1, 3, 29, 31, 32, 64};
  const int Ts[] = {1, 7, 150, 1023, 1024, 1025, 2 * 1024 + 37};
  for (int dtype = 0; dtype < 3; ++dtype)
    for (int V : Vs)
      for (int T : Ts)
        for (int len_mode = 0; len_mode < 3; ++len_mode) {
          one_case(seed, dtype, 1 + (int)(seed % 4), T, V, (int)(seed % 2) ? V - 1 : 0, dtype ? -0.5f : -0.510825634f, len_mode);
          ++seed; ++cases;
        }
  // rows wider than a gather tile (one row per tile), and a bound nothing exceeds / everything exceeds
  one_case(seed++, 0, 2, 5, 9000, 17, -0.5f, 0); ++cases;
  one_case(seed++, 0, 3, 40, 29, 0, INFINITY, 1); ++cases;
  one_case(seed++, 2, 3, 40, 29, 0, -INFINITY, 1); ++cases;
  std::printf("blank_skip_host_main: %u cases, %d failures\n", cases, g_fail);
  return g_fail ? 1 : 0;
}
