// Stand-alone driver of the host twin of the blank-frame filter of live streams (stream_blank_skip_host.cpp), for a sanitizer build on
// the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/native/stream_blank_skip_host_main.cpp -o stream_blank_skip_host_main && ./stream_blank_skip_host_main
// Seeded streams of every dtype are cut into chunks of many sizes (zero-length chunks and ragged seq_lens among them) and fed through
// the scan with carry into exactly-sized heap maps; the map and the counts are compared with a loop over the whole concatenation
// written here from the definition alone.  Both remaps run on exactly-sized buffers; words the definition does not name must keep
// their sentinels.  Test infrastructure only.
#include "stream_blank_skip_host.cpp"

#include <cstdio>
#include <random>

namespace {

int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (++g_fail < 20) { std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

float widen(int dtype, const void *rows, size_t i) {
  if (dtype == 0) return ((const float *)rows)[i];
  return dtype == 1 ? ctcskip::widen_at<1>(rows, i) : ctcskip::widen_at<2>(rows, i);
}

// one stream of N frames, V labels, cut by `cut`(frames left) -> chunk length; every chunk is one call with B = 2: the stream and a
// second stream that sees only the first half of every chunk (ragged seq_lens)
template <typename Cut> void run_stream(int dtype, int N, int V, int blank_id, float c, unsigned seed, Cut cut) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> u(-3.f, 0.f);
  const size_t eb = dtype == 0 ? 4 : 2;
  std::vector<unsigned char> all((size_t)N * V * eb);
  for (size_t i = 0; i < (size_t)N * V; ++i) {
    const float f = u(rng);
    uint32_t w;
    memcpy(&w, &f, 4);
    if (dtype == 0) memcpy(&all[i * 4], &w, 4);
    else { const uint16_t h = dtype == 2 ? (uint16_t)(w >> 16) : (uint16_t)(0xb800u + (w >> 12 & 0x7ffu)); memcpy(&all[i * 2], &h, 2); }
  }
  // the definition on the whole: stream 0 sees every frame, stream 1 the first half of every chunk
  std::vector<int32_t> want0, want1;
  for (int t = 0; t < N; ++t)
    if (!(widen(dtype, all.data(), (size_t)t * V + blank_id) > c)) want0.push_back(t);
  long long frames[2] = {0, 0}, seen[2] = {0, 0};
  std::vector<int32_t> map0, map1;  // exactly frames + chunk length entries before every call
  int at = 0, calls = 0;
  while (at < N || calls == 0) {
    const int T = cut(N - at, calls);
    const int Tb = T < 1 ? 1 : T;  // (a zero-length chunk: a buffer of one frame, seq_lens 0)
    const int32_t lens[2] = {T, T / 2};
    std::vector<unsigned char> rows((size_t)2 * Tb * V * eb, 0x5a);
    if (T > 0) {
      memcpy(&rows[0], &all[(size_t)at * V * eb], (size_t)T * V * eb);
      memcpy(&rows[(size_t)Tb * V * eb], &all[(size_t)at * V * eb], (size_t)T * V * eb);
    }
    for (int t = 0; t < T / 2; ++t)
      if (!(widen(dtype, all.data(), (size_t)(at + t) * V + blank_id) > c)) want1.push_back((int32_t)seen[1] + t);
    std::vector<int32_t> n0(map0.begin(), map0.begin() + frames[0]), n1(map1.begin(), map1.begin() + frames[1]);
    n0.resize((size_t)frames[0] + lens[0], -7);
    n1.resize((size_t)frames[1] + lens[1], -7);
    map0.swap(n0);
    map1.swap(n1);
    int32_t *maps[2] = {map0.data(), map1.data()};
    std::vector<int32_t> kept((size_t)2 * Tb, -9), kl(2, -1);
    const long long f0 = frames[0];
    const int rc = ctcsskip_host_chunk(rows.data(), dtype, lens, 2, Tb, V, blank_id, c, maps, frames, seen, kept.data(), kl.data());
    EXPECT(rc == 0, "chunk call refused");
    EXPECT(kl[0] >= 0 && kl[0] <= T && kl[1] >= 0 && kl[1] <= T / 2, "counts %d %d of %d", kl[0], kl[1], T);
    for (int i = 0; i < kl[0]; ++i) EXPECT(kept[i] == map0[f0 + i] - (int32_t)(seen[0] - T), "chunk-local index %d", i);
    for (int i = kl[0]; i < Tb; ++i) EXPECT(kept[i] == -9, "kept[%d] written beyond n'", i);
    for (size_t i = (size_t)frames[0]; i < map0.size(); ++i) EXPECT(map0[i] == -7, "map written beyond the kept frames");
    at += T;
    ++calls;
    if (calls > 100000) break;
  }
  EXPECT(seen[0] == N, "seen %lld of %d", seen[0], N);
  EXPECT((size_t)frames[0] == want0.size() && (size_t)frames[1] == want1.size(), "kept %lld / %lld want %zu / %zu", frames[0], frames[1], want0.size(), want1.size());
  for (size_t i = 0; i < want0.size() && i < (size_t)frames[0]; ++i) EXPECT(map0[i] == want0[i], "map0[%zu] = %d want %d", i, map0[i], want0[i]);
  for (size_t i = 0; i < want1.size() && i < (size_t)frames[1]; ++i) EXPECT(map1[i] == want1[i], "map1[%zu] = %d want %d", i, map1[i], want1[i]);
}

void remaps() {
  std::mt19937 rng(5);
  const int B = 3, K = 4, stride = 9;
  const int32_t frames[3] = {6, 0, 3};
  std::vector<int32_t> m0 = {2, 5, 70000, 70001, 70010, 90000}, m2 = {1, 2, 3};
  const int32_t *maps[3] = {m0.data(), nullptr, m2.data()};
  // padded rows with a `since` per item: the reported part of a row is [0, len - since)
  std::vector<int32_t> ts((size_t)B * K * stride, 77), lens((size_t)B * K), since = {1, 0, 0}, want;
  for (int b = 0; b < B; ++b)
    for (int p = 0; p < K; ++p) {
      lens[b * K + p] = (int32_t)(rng() % (stride + 2));  // (one beyond the stride too: clamped)
      for (int i = 0; i < stride; ++i) ts[((size_t)b * K + p) * stride + i] = (int32_t)(rng() % 8) - 1;  // -1 and 6, 7: no index of a decoded frame
    }
  want = ts;
  for (int b = 0; b < B; ++b)
    for (int p = 0; p < K; ++p) {
      int n = lens[b * K + p] - since[b];
      n = n < 0 ? 0 : (n > stride ? stride : n);
      for (int i = 0; i < n; ++i) {
        int32_t &w = want[((size_t)b * K + p) * stride + i];
        if (w >= 0 && w < frames[b]) w = maps[b][w];
      }
    }
  ctcsskip_host_remap_rows(ts.data(), nullptr, lens.data(), since.data(), maps, frames, B, K, stride);
  EXPECT(ts == want, "row remap");
  // rows of their own per item (one row each, exactly sized)
  std::vector<int32_t> r0 = {0, 1, 5}, r2 = {2, 9};
  int32_t *rows[3] = {r0.data(), nullptr, r2.data()};
  const int32_t l1[3] = {3, 0, 2};
  ctcsskip_host_remap_rows(nullptr, rows, l1, nullptr, maps, frames, B, 1, 3);
  EXPECT(r0[0] == 2 && r0[1] == 5 && r0[2] == 90000 && r2[0] == 3 && r2[1] == 9, "rows of their own");
  // compact records: item 0 owns labels [1, 5), item 2 labels [5, 7); record 0 and the last are nobody's
  std::vector<uint32_t> lab = {9u | 1u << 16, 1u | 0u << 16, 2u | 1u << 16, 3u | 2u << 16, 4u | 9u << 16, 5u | 2u << 16, 6u | 3u << 16, 7u | 0u << 16};
  const std::vector<uint32_t> before = lab;
  std::vector<int32_t> hdr = {2, 4, 1, 0, 0, 0, 5, 0, 1, 2, 5, 0}, ent((size_t)B * K * 4, 0);
  const int32_t e00[4] = {0, 0, 3, 1}, e01[4] = {1, 2, 3, 4}, e20[4] = {0, 0, 3, 5};  // (e20 claims 3 labels, its item holds 2)
  memcpy(&ent[0], e00, 16);
  memcpy(&ent[4], e01, 16);
  memcpy(&ent[(size_t)2 * K * 4], e20, 16);
  ctcsskip_host_remap_compact(hdr.data(), ent.data(), lab.data(), maps, frames, B, K);
  EXPECT(lab[0] == before[0] && lab[7] == before[7], "records outside every item's range");
  EXPECT(lab[1] == (1u | 2u << 16) && lab[2] == (2u | 5u << 16), "item 0, entry 0");
  EXPECT(lab[3] == before[3], "a frame whose image does not fit 16 bits is left alone");
  EXPECT(lab[4] == before[4], "frame 9 is no decoded frame");
  EXPECT(lab[5] == (5u | 3u << 16) && lab[6] == before[6], "item 2: frame 2 -> 3, frame 3 is beyond its 3 frames");
}

}  // namespace

int main() {
  const int sizes[] = {1, 3, 63, 64, 65, 1023, 1024, 1025};
  for (int dtype = 0; dtype < 3; ++dtype) {
    for (int s : sizes) run_stream(dtype, 2300, dtype ? 7 : 5, dtype, -1.4f, 11u + (unsigned)s, [s](int left, int) { return left < s ? left : s; });
    // zero-length chunks between chunks of changing sizes
    run_stream(dtype, 3000, 6, 2, -1.6f, 3u, [](int left, int call) { const int s = call % 3 == 1 ? 0 : 1 + (call * 389) % 1500; return left < s ? left : s; });
    run_stream(dtype, 0, 4, 0, -1.f, 1u, [](int, int) { return 0; });
  }
  remaps();
  EXPECT(ctcsskip_host_map_grown_cap(0, 1) == 256 && ctcsskip_host_map_grown_cap(256, 257) == 512 && ctcsskip_host_map_grown_cap(512, 5000) == 8192, "map growth");
  EXPECT(ctcsskip_host_compact_route_ok(65536 - 50, 50) == 1 && ctcsskip_host_compact_route_ok(65536 - 49, 50) == 0, "compact route bound");
  if (g_fail) { std::fprintf(stderr, "%d failures\n", g_fail); return 1; }
  std::printf("stream_blank_skip_host_main: ok\n");
  return 0;
}
