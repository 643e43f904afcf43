// Stand-alone driver of the commit's host twin (commit_host.cpp), for a sanitizer build on the CPU:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -mfma -DCTC_ASSUME_CHECKED -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/native/commit_host_main.cpp -o commit_host_main -lpthread && ./commit_host_main
// Streams of random and of peaked rows are fed in ragged chunks from a small frames_hint (the pool doubles), committed and
// compacted in both orders, peeked, and ended; the committed labels followed by the ended stream's best row must be as long as the
// row of a stream that was never committed, label for label.  Test infrastructure only.
#include "commit_host.cpp"

#include <cstdio>
#include <random>

namespace {

std::vector<float> rows_of(int T, int V, unsigned seed, bool peaked) {
  std::mt19937 rng(seed);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<float> x((size_t)T * V);
  int hold = 0, c = 0;
  for (int t = 0; t < T; ++t) {
    if (peaked && hold == 0) { hold = 1 + (int)(rng() % 4); c = (rng() & 1) ? 0 : (int)(rng() % V); }
    double sum = 0.0;
    for (int v = 0; v < V; ++v) {
      float z = nd(rng);
      if (peaked && v == c) z += 12.f;
      x[(size_t)t * V + v] = z;
      sum += std::exp((double)z);
    }
    for (int v = 0; v < V; ++v) x[(size_t)t * V + v] -= (float)std::log(sum);
    if (hold) --hold;
  }
  return x;
}

struct Result { std::vector<int32_t> tok, ts; int len = 0; };

// one stream over `rows`; mode 0: never committed, 1: commit after every chunk, 2: commit then compact, 3: compact then commit
int run(const std::vector<float> &rows, int T, int V, int beam, int mode, Result *res) {
  void *h = ctccompact_host_create(V, beam, 4, 1.0, 40, 0, 0.0, 0.0, nullptr, nullptr, mode == 3 ? 1 : 0);
  if (!h) return 1;
  void *inner = ctccompact_host_inner(h);
  std::vector<int32_t> ctok((size_t)T + 1), cts((size_t)T + 1), all_tok, all_ts;
  const int chunks[] = {0, 7, 1, 30, 0, 33, 64, 5};
  int fed = 0, rc = 0;
  for (size_t c = 0; fed < T && !rc; ++c) {
    int len = chunks[c % 8];
    if (fed + len > T) len = T - fed;
    const bool end = fed + len == T;
    std::vector<int32_t> tok((size_t)beam * T), ts((size_t)beam * T), lens(beam);
    std::vector<float> sc(beam);
    int32_t nres = 0;
    if (ctccompact_host_prepare(h, len) != 0) { rc = 2; break; }
    if (ctcpeek_host_feed(inner, rows.data() + (size_t)fed * V, len, end ? 1 : 0, tok.data(), ts.data(), sc.data(), lens.data(), &nres, T) != 1) { rc = 3; break; }
    fed += len;
    if (end) {
      res->tok = all_tok; res->ts = all_ts;
      res->tok.insert(res->tok.end(), tok.begin(), tok.begin() + lens[0]);
      res->ts.insert(res->ts.end(), ts.begin(), ts.begin() + lens[0]);
      res->len = (int)res->tok.size();
      break;
    }
    if (mode == 0) continue;
    if (mode == 3 && ctccompact_host_compact(h) < 0) { rc = 4; break; }
    int live = 0;
    const int m = ctccommit_host_commit(h, ctok.data(), cts.data(), T, &live);
    if (m < 0) { rc = 5; break; }
    all_tok.insert(all_tok.end(), ctok.begin(), ctok.begin() + m);
    all_ts.insert(all_ts.end(), cts.begin(), cts.begin() + m);
    if (fed > 0 && (ctccompact_host_pool_count(h) != live || !ctccompact_host_parents_below(h))) { rc = 6; break; }
    if (mode == 2 && ctccompact_host_compact(h) != live) { rc = 7; break; }
    const unsigned long long d0 = ctccompact_host_digest(h);
    if (ctccommit_host_commit(h, ctok.data(), cts.data(), T, &live) != 0 || ctccompact_host_digest(h) != d0) { rc = 8; break; }
    std::vector<int32_t> ptok((size_t)beam * (fed + 1)), pts((size_t)beam * (fed + 1)), plen(beam);
    std::vector<float> psc(beam);
    int32_t pn = 0, stable = 0;
    if (ctcpeek_host_peek(inner, beam, 0, ptok.data(), pts.data(), fed + 1, psc.data(), plen.data(), &pn, &stable, nullptr) != 1) { rc = 9; break; }
    if (fed > 0 && m > 0 && stable != 1) { rc = 10; break; }  // (all of the common prefix but its last label has just left)
  }
  ctccompact_host_destroy(h);
  return rc;
}

}  // namespace

int main() {
  int bad = 0;
  long long committed = 0;
  for (int peaked = 0; peaked < 2; ++peaked)
    for (int beam : {1, 8, 30}) {
      const int T = 400, V = 11;
      const std::vector<float> rows = rows_of(T, V, 17u + (unsigned)beam + 100u * (unsigned)peaked, peaked != 0);
      Result plain;
      if (int rc = run(rows, T, V, beam, 0, &plain)) { std::printf("beam %d: the plain stream failed (%d)\n", beam, rc); ++bad; continue; }
      for (int mode = 1; mode <= 3; ++mode) {
        Result r;
        const int rc = run(rows, T, V, beam, mode, &r);
        const bool same = rc == 0 && r.tok == plain.tok && r.ts == plain.ts;
        if (!same) { std::printf("peaked %d beam %d mode %d: rc %d, %d labels against %d\n", peaked, beam, mode, rc, r.len, plain.len); ++bad; }
      }
      committed += plain.len;
    }
  std::printf("%s (%lld labels in the plain rows)\n", bad ? "FAILED" : "ok", committed);
  return bad ? 1 : 0;
}
