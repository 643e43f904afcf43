// A program of its own for the sanitizers (-fsanitize=address,undefined; never loaded into another process): the host twin of the
// stream images (snapshot_host.cpp) driven through save / restore, then snapshot_check fed one valid image and systematic mutations
// of it.  Every mutation the check accepts is looked at a second time by a check written here, independently: an accepted image with
// a pool index outside [-1, M), a parent not below its node, or an order word outside [0, n) fails the run.  Test infrastructure only.
#include "snapshot_host.cpp"

#include <cstdio>
#include <cstdlib>

namespace {

struct Rng {
  unsigned long long s;
  unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
  float uni() { return (float)(next() & 0xFFFFFF) / (float)0x1000000; }
};

// transcript-like rows: a label or the blank dominates for a few frames
std::vector<float> rows(int T, int V, unsigned long long seed) {
  Rng r{seed};
  std::vector<float> x((size_t)T * V);
  int t = 0;
  while (t < T) {
    const int n = 1 + (int)(r.next() % 4), c = (r.next() & 1) ? 0 : (int)(r.next() % (unsigned)V);
    const float boost = r.uni() < 0.4f ? 1.0f : 12.0f;
    for (int i = 0; i < n && t < T; ++i, ++t) {
      float m = -1e30f;
      for (int v = 0; v < V; ++v) { x[(size_t)t * V + v] = 2.f * r.uni() + (v == c ? boost : 0.f); m = std::max(m, x[(size_t)t * V + v]); }
      double sum = 0;
      for (int v = 0; v < V; ++v) sum += std::exp((double)(x[(size_t)t * V + v] - m));
      for (int v = 0; v < V; ++v) x[(size_t)t * V + v] = x[(size_t)t * V + v] - m - (float)std::log(sum);
    }
  }
  return x;
}

struct Result {
  std::vector<int32_t> tok, ts, len;
  std::vector<float> sc;
  int32_t n = 0;
  bool operator==(const Result &o) const { return tok == o.tok && ts == o.ts && len == o.len && n == o.n && memcmp(sc.data(), o.sc.data(), sc.size() * 4) == 0; }
};

void *make(int V, int K, int hint) { return ctccompact_host_create(V, K, hint, 1.0, 40, 0, 0.0, 0.0, nullptr, nullptr, 0); }

bool feed(void *c, const float *r, int len, int V, int K, int total, Result *out) {
  if (ctccompact_host_prepare(c, len) != 0) return false;
  Result res;
  res.tok.assign((size_t)K * total, 0); res.ts.assign((size_t)K * total, 0); res.len.assign((size_t)K, 0); res.sc.assign((size_t)K, 0.f);
  (void)V;
  const int rc = ctcpeek_host_feed(ctccompact_host_inner(c), r, len, out ? 1 : 0, res.tok.data(), res.ts.data(), res.sc.data(), res.len.data(), &res.n, total);
  if (out) *out = res;
  return rc == 1;
}

std::vector<unsigned char> save(void *c) {
  const long long n = ctcsnap_host_save(c, 0, nullptr, 0);
  std::vector<unsigned char> b((size_t)(n > 0 ? n : 0));
  if (n <= 0 || ctcsnap_host_save(c, 0, b.data(), n) != n) { std::printf("save failed\n"); std::exit(2); }
  return b;
}

// the second pass: ranges only, from the format's description
bool indices_in_range(const std::vector<unsigned char> &img, int K, int A) {
  const int32_t *w = (const int32_t *)img.data();  // (a std::vector's storage: aligned)
  const int M = w[12], n = w[16 + 1];
  const long long frames = (long long)(uint32_t)w[8] | ((long long)w[9] << 32);
  const int32_t *arr = w + 16 + 12, *node = arr + (size_t)A * K, *up = node + (size_t)3 * M;
  if (node[0] != -1) return false;
  for (int i = 1; i < M; ++i)
    if (node[3 * i] < 0 || node[3 * i] >= i || up[i] < 0 || up[i] > i) return false;
  if (frames == 0) return true;
  if (n < 1 || n > K) return false;
  const int idx[5] = {0, 1, 5, 6, 8};
  for (int j = 0; j < n; ++j) {
    for (int a : idx)
      if (arr[(size_t)a * K + j] < -1 || arr[(size_t)a * K + j] >= M) return false;
    if (arr[(size_t)13 * K + j] < 0 || arr[(size_t)13 * K + j] >= n) return false;
  }
  return true;
}

}  // namespace

int main() {
  const int V = 29, K = 20, T = 150;
  const std::vector<float> x = rows(T, V, 12345);
  // 1. save / restore between chunks, against the stream that is never saved
  Result plain, moved;
  {
    void *a = make(V, K, T + 1);
    if (!feed(a, x.data(), T, V, K, T, &plain)) return 3;
    ctccompact_host_destroy(a);
  }
  std::vector<unsigned char> good;
  void *cur = make(V, K, 4);
  for (int lo = 0; lo < T; lo += 50) {
    const bool end = lo + 50 >= T;
    if (!feed(cur, x.data() + (size_t)lo * V, 50, V, K, T, end ? &moved : nullptr)) return 4;
    if (end) break;
    const std::vector<unsigned char> img = save(cur);
    if (save(cur) != img) { std::printf("a second save gives other bytes\n"); return 5; }
    void *next = make(V, K, 1);
    long long committed = -1;
    if (ctcsnap_host_restore(next, img.data(), (long long)img.size(), lo == 0 ? 4 : 500, &committed) != 0 || committed != 0) return 6;
    if (save(next) != img) { std::printf("save -> restore -> save gives other bytes\n"); return 7; }
    ctccompact_host_destroy(cur);
    cur = next;
    good = img;
  }
  if (!(plain == moved)) { std::printf("the restored stream ends with another result\n"); return 8; }
  std::printf("save/restore walk ok, image %zu bytes\n", good.size());

  // 2. the check under mutations
  const ctcsnap::SnapExpect ex = expect_of(*((CompactStream *)cur)->s);
  const int A = ctcbeam::kStateArrays;
  const size_t nwords = good.size() / 4, head = ctcsnap::snapshot_head_words(K, 0);
  const int M = ((const int32_t *)good.data())[12];
  if (ctcsnap::snapshot_check(good.data(), good.size(), ex) != ctcsnap::SNAP_OK || !indices_in_range(good, K, A) || M < 64) return 9;
  long long tried = 0, accepted = 0, bad = 0;
  auto probe = [&](const std::vector<unsigned char> &img, size_t bytes) {
    ++tried;
    // (an exact-size heap copy: a read behind the image is the sanitizer's to report)
    unsigned char *p = (unsigned char *)std::malloc(bytes ? bytes : 1);
    memcpy(p, img.data(), bytes);
    const int code = ctcsnap::snapshot_check(p, bytes, ex);
    std::free(p);
    if (code != ctcsnap::SNAP_OK) return;
    ++accepted;
    if (bytes != img.size() || !indices_in_range(img, K, A)) ++bad;
  };
  auto with_word = [&](size_t i, int32_t v) {
    std::vector<unsigned char> m = good;
    memcpy(m.data() + i * 4, &v, 4);
    probe(m, m.size());
  };
  const int32_t *gw = (const int32_t *)good.data();
  const int32_t deltas[] = {1, -1, 2, 1 << 16, (int32_t)0x80000000u, 0x7fffffff};
  for (size_t i = 0; i < (size_t)ctcsnap::SNAP_HDR_WORDS + ctcbeam::SH_WORDS; ++i) {  // every header word perturbed
    for (int32_t dlt : deltas) with_word(i, (int32_t)((uint32_t)gw[i] + (uint32_t)dlt));
    with_word(i, 0); with_word(i, -1);
  }
  for (size_t wd = 0; wd <= head; ++wd) probe(good, wd * 4);  // truncation at every word boundary of the head
  for (size_t k = 1; k <= 40; ++k) probe(good, (head + (nwords - head) * k / 41) * 4);  // ... and inside the node part
  for (size_t odd : {(size_t)1, (size_t)3, good.size() - 1, good.size() - 3}) probe(good, odd);
  Rng r{777};
  const int idx_arrays[] = {0, 1, 3, 4, 5, 6, 8, 13};
  const int32_t values[] = {-2, -1, 0, 1, M - 1, M, M + 1, K, K + 1, 0x7fffffff, (int32_t)0x80000000u, 65536};
  for (int it = 0; it < 6000; ++it) {  // seeded single-word corruptions of the index-bearing words
    size_t i;
    const unsigned kind = r.next() % 3;
    if (kind == 0) i = (size_t)ctcsnap::SNAP_HDR_WORDS + ctcbeam::SH_WORDS + (size_t)idx_arrays[r.next() % 8] * K + r.next() % (unsigned)K;
    else if (kind == 1) i = head + 3 * (size_t)(r.next() % (unsigned)M);          // a parent
    else i = head + 3 * (size_t)M + (size_t)(r.next() % (unsigned)M);             // an express word
    const unsigned pick = r.next() % 16;
    with_word(i, pick < 12 ? values[pick] : (int32_t)(r.next() % (unsigned)(M + 3)) - 1);
  }
  std::printf("mutations %lld accepted %lld accepted-with-bad-index %lld\n", tried, accepted, bad);
  ctccompact_host_destroy(cur);
  return bad == 0 && tried > 6000 ? 0 : 10;
}
