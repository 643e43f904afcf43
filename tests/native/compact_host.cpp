// Host twin of the stream compaction (ctcdecode_amd/csrc/stream_compact.h): the stream of peek_host.cpp -- the host build of the
// core fed chunk by chunk, the peek run on its parked state -- with the compaction run on that state between chunks under a
// sequential policy, and the capacity bookkeeping of the product (struct ctcd_stream, stream_prepare) on the header's arithmetic.
// Test infrastructure only.  (peek_host.cpp, and core_host.cpp through it, are compiled into this library as they are.)
#include "peek_host.cpp"

#include "../../ctcdecode_amd/csrc/stream_compact.h"

namespace {

struct CompactStream {
  PeekStream *s = nullptr;
  long long cap_frames = 0, hint_frames = 0, base_nodes = 1, base_frames = 0;
  long long min_nodes = 0;  // the policy of ctcd_set_stream_compaction (0: off)
  int compactions = 0;
};

// the stream's pool in a block of cap_frames (stream_grow / the move to a smaller block: the first `used` nodes come along)
void resize_pool(CompactStream &c, long long cap_frames, size_t used) {
  PeekStream &s = *c.s;
  const size_t ncap = (size_t)ctccompact::pool_capacity(cap_frames, s.beam), ocap = s.pool.size();
  std::vector<ctcbeam::PoolNode> pool(ncap);
  std::vector<int> up(2 * ncap, 0);
  for (size_t i = 0; i < used; ++i) { pool[i] = s.pool[i]; up[i] = s.pool_up[i]; up[ncap + i] = s.pool_up[ocap + i]; }
  s.pool.swap(pool);
  s.pool_up.swap(up);
  c.cap_frames = cap_frames;
}

int compact(CompactStream &c) {
  using namespace ctcbeam;
  namespace cc = ctccompact;
  PeekStream &s = *c.s;
  cc::CompactWork w;
  std::vector<char> mem(cc::compact_carve(w, nullptr, s.beam) + 64, (char)0x5a);
  cc::compact_carve(w, mem.data(), s.beam);
  HostX x;
  const int cap = (int)s.pool.size();
  const cc::CompactPlan pl = cc::compact_plan(x, w, s.beam, s.hdr.data(), s.arrays.data(), cap);
  if (pl.M < 0) return -1;
  if (pl.M == 0) return 1;  // no frames: the root alone, nothing to do
  std::vector<int> scratch(cc::compact_out_ints(pl.M), 0x5a5a5a5a);
  const cc::CompactOut out = cc::compact_out_at(scratch.data(), pl.M);
  if (cc::compact_gather(x, w, pl, s.beam, s.hdr.data(), s.arrays.data(), s.pool.data(), s.pool_up.data(), cap, out) != cc::COMPACT_OK) return -1;
  const long long nf = cc::shrunk_cap_frames(c.cap_frames, c.hint_frames, pl.M, s.beam);
  if (nf) resize_pool(c, nf, 0);
  cc::compact_write_back(x, pl.M, out, s.hdr.data(), s.hdr.data(), 0, s.pool.data(), s.pool_up.data(), (int)s.pool.size());
  c.base_nodes = pl.M;
  c.base_frames = s.frames;
  ++c.compactions;
  return pl.M;
}

}  // namespace

extern "C" void *ctccompact_host_create(int V, int beam, int frames_hint, double cutoff_prob, int cutoff_top_n, int blank_id, double alpha,
                                        double beta, const char *lm_path, const char *labels, long long min_nodes) {
  PeekStream *s = (PeekStream *)ctcpeek_host_create(V, beam, frames_hint, cutoff_prob, cutoff_top_n, blank_id, alpha, beta, lm_path, labels);
  if (!s) return nullptr;
  CompactStream *c = new CompactStream;
  c->s = s;
  c->cap_frames = c->hint_frames = frames_hint;
  c->min_nodes = min_nodes;
  s->cap_frames = 0x7fffffff;  // (the capacity is kept here, in nodes: ctccompact_host_prepare)
  return c;
}

extern "C" void ctccompact_host_destroy(void *h) {
  CompactStream *c = (CompactStream *)h;
  if (c) ctcpeek_host_destroy(c->s);
  delete c;
}

// the stream of peek_host.cpp inside: ctcpeek_host_feed / ctcpeek_host_peek take it
extern "C" void *ctccompact_host_inner(void *h) { return ((CompactStream *)h)->s; }

// what stream_prepare does before a chunk of `len` frames: the pool doubles until the chunk fits -- with the policy on, a stream
// whose bound has reached min_nodes is compacted first.  Returns 0, or -1 (stream too long for this beam width / bad state).
extern "C" int ctccompact_host_prepare(void *h, int len) {
  namespace cc = ctccompact;
  CompactStream &c = *(CompactStream *)h;
  const PeekStream &s = *c.s;
  long long need = cc::pool_bound(s.frames + len, c.base_nodes, c.base_frames, s.beam);
  if (need > cc::pool_capacity(c.cap_frames, s.beam) && c.min_nodes > 0 && s.frames > c.base_frames &&
      cc::pool_bound(s.frames, c.base_nodes, c.base_frames, s.beam) >= c.min_nodes) {
    if (compact(c) < 0) return -1;
    need = cc::pool_bound(s.frames + len, c.base_nodes, c.base_frames, s.beam);
  }
  if (need > 0x7fffffffLL) return -1;
  if (need > cc::pool_capacity(c.cap_frames, s.beam))
    resize_pool(c, cc::grown_cap_frames(c.cap_frames, need, s.beam), (size_t)cc::pool_bound(s.frames, c.base_nodes, c.base_frames, s.beam));
  return 0;
}

// ctcd_stream_compact for this stream: the nodes it keeps (1: no frames yet), or -1
extern "C" int ctccompact_host_compact(void *h) { return compact(*(CompactStream *)h); }

extern "C" long long ctccompact_host_capacity(const void *h) { return (long long)((const CompactStream *)h)->s->pool.size(); }
extern "C" long long ctccompact_host_bound(const void *h) {
  const CompactStream &c = *(const CompactStream *)h;
  return ctccompact::pool_bound(c.s->frames, c.base_nodes, c.base_frames, c.s->beam);
}
extern "C" int ctccompact_host_pool_count(const void *h) { return ((const CompactStream *)h)->s->hdr[ctcbeam::SH_POOL]; }
extern "C" int ctccompact_host_compactions(const void *h) { return ((const CompactStream *)h)->compactions; }

// 1 when the root has no parent and every other node of the pool has its parent below it
extern "C" int ctccompact_host_parents_below(const void *h) {
  const PeekStream &s = *((const CompactStream *)h)->s;
  const int used = s.hdr[ctcbeam::SH_POOL];
  if (used < 1 || (size_t)used > s.pool.size() || s.pool[0].parent != -1) return 0;
  for (int i = 1; i < used; ++i)
    if (s.pool[i].parent < 0 || s.pool[i].parent >= i) return 0;
  return 1;
}

// checksum of the parked block: header, beam arrays, and nodes, express words and time steps' high parts of the pool count
extern "C" unsigned long long ctccompact_host_digest(const void *h) {
  const PeekStream &s = *((const CompactStream *)h)->s;
  unsigned long long hsh = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t bytes) {
    const unsigned char *c = (const unsigned char *)p;
    for (size_t i = 0; i < bytes; ++i) hsh = (hsh ^ c[i]) * 1099511628211ull;
  };
  mix(s.hdr.data(), s.hdr.size() * 4);
  mix(s.arrays.data(), s.arrays.size() * 4);
  const size_t used = (size_t)s.hdr[ctcbeam::SH_POOL], cap = s.pool.size();
  for (size_t i = 0; i < used && i < cap; ++i) {
    mix(&s.pool[i].parent, 4); mix(&s.pool[i].lpc, 4); mix(&s.pool[i].cht, 4);
    mix(&s.pool_up[i], 4); mix(&s.pool_up[cap + i], 4);
  }
  return hsh;
}
