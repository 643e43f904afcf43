// Host twin of the stream commit (ctcdecode_amd/csrc/stream_commit.h): the stream of compact_host.cpp -- the host build of the core
// fed chunk by chunk, peek and compaction run on its parked state, the product's capacity bookkeeping -- with the commit run on that
// state between chunks under a sequential policy.  Test infrastructure only.  (compact_host.cpp, and peek_host.cpp / core_host.cpp
// through it, are compiled into this library as they are.)
#include "compact_host.cpp"

#include "../../ctcdecode_amd/csrc/stream_commit.h"

// ctcd_stream_commit for this stream: the labels it commits now (tokens / timesteps: room for `cap` of them), or -1 (bad state),
// -2 (a stream with a scorer: refused, nothing is touched), -3 (cap too small: nothing is touched).  *live (if not null): the
// nodes the stream keeps (1: no frames yet).
extern "C" int ctccommit_host_commit(void *h, int32_t *tokens, int32_t *timesteps, int cap, int *live) {
  using namespace ctcbeam;
  namespace cc = ctccompact;
  namespace cm = ctccommit;
  CompactStream &c = *(CompactStream *)h;
  PeekStream &s = *c.s;
  if (s.lm) return -2;
  cc::CompactWork w;
  std::vector<char> mem(cc::compact_carve(w, nullptr, s.beam) + 64, (char)0x5a);
  cc::compact_carve(w, mem.data(), s.beam);
  HostX x;
  const int pcap = (int)s.pool.size();
  const cm::CommitPlan pl = cm::commit_plan(x, w, s.beam, s.hdr.data(), s.arrays.data(), pcap);
  if (pl.cp.M < 0) return -1;
  if (live) *live = pl.cp.M == 0 ? 1 : pl.M;
  if (pl.cp.M == 0) return 0;  // no frames: the root alone, nothing to do
  if (pl.drop > cap) return -3;
  std::vector<int> scratch(cc::compact_out_ints(pl.M), 0x5a5a5a5a);
  std::vector<int32_t> tok((size_t)pl.drop + 1, -7), ts((size_t)pl.drop + 1, -7);
  const cc::CompactOut out = cc::compact_out_at(scratch.data(), pl.M);
  if (cm::commit_gather(x, w, pl, s.beam, s.hdr.data(), s.arrays.data(), s.pool.data(), s.pool_up.data(), pcap, out, tok.data(), ts.data()) != cc::COMPACT_OK)
    return -1;
  const long long nf = cc::shrunk_cap_frames(c.cap_frames, c.hint_frames, pl.M, s.beam);
  if (nf) resize_pool(c, nf, 0);
  cc::compact_write_back(x, pl.M, out, s.hdr.data(), s.hdr.data(), 0, s.pool.data(), s.pool_up.data(), (int)s.pool.size());
  c.base_nodes = pl.M;
  c.base_frames = s.frames;
  ++c.compactions;
  for (int i = 0; i < pl.drop; ++i) { tokens[i] = tok[i]; timesteps[i] = ts[i]; }
  return pl.drop;
}

// the high part of the time step of pool node i (the frame number's bits 16 and up), -1 outside the pool count
extern "C" int ctccommit_host_node_thi(const void *h, int i) {
  const PeekStream &s = *((const CompactStream *)h)->s;
  if (i < 0 || i >= s.hdr[ctcbeam::SH_POOL]) return -1;
  return s.pool_up[s.pool.size() + (size_t)i];
}
