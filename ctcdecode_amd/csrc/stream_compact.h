// stream_compact.h -- compaction of a PARKED stream's node pool (beam_core.h StreamState / save_state): keep exactly the nodes that
// are ancestors of a current beam entry, drop the rest, rewrite every stored pool index.  The pool is append-only and every pool
// access of beam_core.h is a parent or express walk that starts from a beam entry (phase A2's dead-interior lookup, finish()'s and
// the peek's back-trace), so the ancestors of the beam are everything a later chunk, peek or stream end can reach: nothing they
// compute changes.  The reference frees the same nodes as it goes (path_trie.cpp remove()).
//
// The beam is a DFS-ordered list with an LCP array (Beam::lcp: labels entry j shares with entry j - 1), so the live set is the
// root plus, per entry j, the nodes of its path at depths lcp[j] + 1 .. dep[j] (entry 0: its whole path), and the new layout is
// fixed by that alone: root at 0, then entry 0's nodes by increasing depth, then entry 1's own nodes, ...  The node at depth e of
// entry j's path sits at base[j] + e - lcp[j] - 1 when e > lcp[j], else in the block of the nearest earlier entry i with
// lcp[i] < e (e == 0: the root).  No forwarding table over the old pool; the cost follows the live set, not the old pool.
//
// The per-stream routines are written against an execution policy like stream_peek.h: the workgroup of stream_compact.hip on the
// GPU, a sequential one on the host (tests/native/compact_host.cpp).  The capacity arithmetic of a stream (struct ctcd_stream) is
// here as well, HIP-free, so that the host twin grows, compacts and shrinks at the same points as the product.
#pragma once
#include "beam_core.h"

namespace ctccompact {

using namespace ctcbeam;

enum : int { COMPACT_OK = 0, COMPACT_BAD_STATE = 1 };  // status word of one stream (bad: the parked state is not one save_state wrote; nothing of it is changed)

// positions of the arrays of a parked state that hold pool indices (save_state: arrays[a * K + i]), and of the two that say where
enum { CA_NODE = 0, CA_PAR = 1, CA_DEP = 3, CA_LCP = 4, CA_VIA = 5, CA_VIAANC = 6, CA_UP = 8 };

// ---- a stream's capacity arithmetic (host) --------------------------------------------------------------------------------------
// A pool holds cap_frames * beam + 1 nodes.  An uncompacted stream can have filled frames * beam + 1 of them; after a compaction
// that left base_nodes at frame base_frames the bound is base_nodes + (frames - base_frames) * beam.  (1, 0) before the first
// compaction: the arithmetic of a stream that is never compacted is the one it always had.
inline long long pool_capacity(long long cap_frames, int beam) { return cap_frames * beam + 1; }
inline long long pool_bound(long long frames, long long base_nodes, long long base_frames, int beam) { return base_nodes + (frames - base_frames) * beam; }
// growth by doubling: the smallest cap_frames * 2^k (k >= 1) whose pool takes `need` nodes
inline long long grown_cap_frames(long long cap_frames, long long need, int beam) {
  long long cap = cap_frames * 2;
  while (pool_capacity(cap, beam) < need) cap *= 2;
  return cap;
}
// after a compaction that left M nodes: the stream asks for max(capacity of its frames_hint, 2 * M) nodes, and moves to a block
// of that size only when that is at most a quarter of what it has.  Returns the new cap_frames, or 0: the stream keeps its block.
inline long long shrunk_cap_frames(long long cap_frames, long long hint_frames, long long M, int beam) {
  const long long for_2m = (2 * M - 1 + beam - 1) / beam;  // (capacities are whole frames: the first one that takes 2 * M nodes)
  const long long want = hint_frames > for_2m ? hint_frames : for_2m;
  return 4 * pool_capacity(want, beam) <= pool_capacity(cap_frames, beam) ? want : 0;
}

// ---- the per-stream routines ----------------------------------------------------------------------------------------------------
constexpr int kCompactThreads = 256;  // threads of a workgroup at most (the size of the reduction arrays)
constexpr int kCompactBlk = 64;       // entries per block of the minima the shared-node lookup skips by

// Scratch of one stream (LDS on the GPU)
struct CompactWork {
  int *base;        // K: new index of the first node entry j owns
  int *lo;          // K: the depth below which entry j's path belongs to earlier entries (lcp[j], 0 for entry 0)
  int *blkmin;      // K / kCompactBlk + 1: min(lo) per block of entries
  long long *part;  // kCompactThreads: the threads' node counts
  int *pmax;        // kCompactThreads: the threads' deepest entry
  int *vars;        // CV_COUNT
};
enum { CV_BAD = 0, CV_COUNT = 4 };
CTC_HD size_t compact_carve(CompactWork &w, char *base, int K) {
  char *p = base;
  w.part = carve_ptr<long long>(p, (size_t)kCompactThreads);
  w.base = carve_ptr<int>(p, (size_t)K);
  w.lo = carve_ptr<int>(p, (size_t)K);
  w.blkmin = carve_ptr<int>(p, (size_t)K / kCompactBlk + 1);
  w.pmax = carve_ptr<int>(p, (size_t)kCompactThreads);
  w.vars = carve_ptr<int>(p, CV_COUNT);
  return (size_t)(p - base);
}

// the new layout of one stream: M nodes (12 bytes each), their express words, the high parts of their time steps
struct CompactOut {
  PoolNode *node;
  int *up, *thi;
};
CTC_HD size_t compact_out_ints(long long M) { return (size_t)M * 5; }
CTC_HD CompactOut compact_out_at(int *scratch, long long M) {
  CompactOut o;
  o.node = reinterpret_cast<PoolNode *>(scratch);
  o.up = scratch + (size_t)M * 3;
  o.thi = scratch + (size_t)M * 4;
  return o;
}

struct CompactPlan {
  int n;        // beam entries
  int M;        // nodes of the live set, root included (0: the stream has no frames -- nothing to do; -1: bad state)
  int maxdep;   // the deepest entry
};

CTC_HD int compact_dep(const int *arrays, int K, int j) {
  const int d = arrays[(size_t)CA_DEP * K + j];
  return d < 0 ? 0 : d;
}

// The layout: lo[], base[], blkmin[] and the node count.  X: tid(), nt() (<= kCompactThreads), sync() (a barrier that also orders
// global memory), uni().  Identical in every thread.
template <class X>
CTC_HD CompactPlan compact_plan(X &x, const CompactWork &w, int K, const int *hdr, const int *arrays, int pool_cap) {
  const int tid = x.tid(), nt = x.nt();
  CompactPlan pl;
  pl.n = 0; pl.M = 0; pl.maxdep = 0;
  if (x.uni(hdr[SH_FRAMES]) <= 0) return pl;  // zeroed memory, or parked by empty chunks only: the root alone
  int n = x.uni(hdr[SH_N]);
  n = n < 1 ? 1 : (n > K ? K : n);  // (1 <= n <= K in every parked state)
  pl.n = n;
  const int *lcp = arrays + (size_t)CA_LCP * K;
  const int per = (n + nt - 1) / nt, j0 = tid * per, j1 = j0 + per < n ? j0 + per : n;  // a run of consecutive entries per thread
  long long own = 0;
  int deepest = 0;
  for (int j = j0; j < j1; ++j) {
    const int d = compact_dep(arrays, K, j);
    int l = j == 0 ? 0 : lcp[j];
    l = l < 0 ? 0 : (l > d ? d : l);
    w.lo[j] = l;
    own += d - l;
    deepest = d > deepest ? d : deepest;
  }
  w.part[tid] = own;
  w.pmax[tid] = deepest;
  if (tid == 0) w.vars[CV_BAD] = 0;
  x.sync();
  long long before = 0, total = 0;
  for (int t = 0; t < nt; ++t) {
    const long long v = w.part[t];
    before += t < tid ? v : 0;
    total += v;
    deepest = w.pmax[t] > deepest ? w.pmax[t] : deepest;
  }
  pl.maxdep = deepest;
  const long long M = 1 + total;
  // the live nodes are distinct nodes of the pool: more of them than the pool holds is no state that save_state wrote
  const int used = x.uni(hdr[SH_POOL]);
  if (M > (long long)pool_cap || M > (long long)used) { pl.M = -1; return pl; }
  pl.M = (int)M;
  int run = (int)(1 + before);
  for (int j = j0; j < j1; ++j) {
    w.base[j] = run;
    run += compact_dep(arrays, K, j) - w.lo[j];
  }
  for (int blk = tid; blk * kCompactBlk < n; blk += nt) {
    int m = kIntMax;
    const int e1 = (blk + 1) * kCompactBlk < n ? (blk + 1) * kCompactBlk : n;
    for (int j = blk * kCompactBlk; j < e1; ++j) m = w.lo[j] < m ? w.lo[j] : m;
    w.blkmin[blk] = m;
  }
  x.sync();
  return pl;
}

// New index of the node at depth e of entry j's path.  e <= lo[j]: the nearest earlier entry i with lo[i] < e owns it (every entry
// between i and j shares at least e labels with its predecessor, so the paths agree down to depth e); lo[0] == 0 ends the search.
// Whole blocks of entries whose minimum is not below e are skipped.
CTC_HD int compact_index(const CompactWork &w, int M, int j, int e) {
  if (e <= 0) return 0;
  int i = j;
  if (e <= w.lo[j]) {
    i = j - 1;
    while (i > 0 && w.lo[i] >= e) {
      if ((i & (kCompactBlk - 1)) == 0) {
        int blk = i / kCompactBlk - 1;
        while (blk > 0 && w.blkmin[blk] >= e) --blk;
        i = blk * kCompactBlk + kCompactBlk - 1;
      } else {
        --i;
      }
    }
    if (i < 0) i = 0;
  }
  const int q = w.base[i] + e - w.lo[i] - 1;
  return (unsigned)q < (unsigned)M ? q : 0;  // (outside the layout: a state no save_state wrote; the index stays inside the pool)
}

// Gathers the live set of one stream into `out` (the new layout), then rewrites the parked beam arrays that hold pool indices and
// the pool count IN the block.  The old pool is only read.  pool_up: express pointers, then the time steps' high parts at pool_up +
// pool_cap.  Tasks are (entry, segment of kExpress hops) pairs reached through the express pointers as in finish() and the peek
// (segment 0: the tail above the node's express ancestor, segment i >= 1 the kExpress labels below the i-th express ancestor), one
// thread each, segment-major: a path of depth 3000 is ~94 independent walks.  Only the segments an entry owns nodes in are walked.
// Returns COMPACT_OK or COMPACT_BAD_STATE (identical in every thread; bad: a walk left the pool -- the block is unchanged).
template <class X>
CTC_HD int compact_gather(X &x, const CompactWork &w, const CompactPlan &pl, int K, int *hdr, int *arrays, const PoolNode *pool,
                          const int *pool_up, int pool_cap, const CompactOut &out) {
  const int tid = x.tid(), nt = x.nt();
  const int n = pl.n, M = pl.M;
  const int *pool_thi = pool_up + pool_cap;
  int *b_node = arrays + (size_t)CA_NODE * K, *b_par = arrays + (size_t)CA_PAR * K, *b_up = arrays + (size_t)CA_UP * K;
  int *b_via = arrays + (size_t)CA_VIA * K, *b_viaanc = arrays + (size_t)CA_VIAANC * K;
  if (tid == 0) {
    if (pool_cap > 0) {
      PoolNode r = pool[0];
      r.parent = -1;
      out.node[0] = r; out.up[0] = 0; out.thi[0] = pool_thi[0];
    } else {
      w.vars[CV_BAD] = 1;
    }
  }
  const long long nseg = (long long)pl.maxdep / kExpress + 1;
  for (long long idx = tid; idx < nseg * n; idx += nt) {
    const int i = (int)(idx / n), j = (int)(idx - (long long)i * n);
    const int dj = compact_dep(arrays, K, j), lo = w.lo[j];
    const int top = ((dj - 1) / kExpress) * kExpress;  // depth of the first express ancestor
    if (dj <= lo || i > top / kExpress) continue;
    int dd = i == 0 ? dj : top - (i - 1) * kExpress;
    int stop = i == 0 ? top : dd - kExpress;
    if (dd <= lo) continue;  // (below what the entry owns: nothing of the segment is fetched)
    stop = stop < lo ? lo : stop;
    int xn;
    if (i == 0) {
      xn = b_node[j];
    } else {
      xn = b_up[j];
      for (int h = 1; h < i && (unsigned)xn < (unsigned)pool_cap; ++h) xn = pool_up[xn];
    }
    const int q0 = w.base[j] - lo - 1;  // entry j's node of depth e goes to q0 + e
    while (dd > stop) {
      if ((unsigned)xn >= (unsigned)pool_cap) { w.vars[CV_BAD] = 1; break; }  // (a node index outside the pool is not followed)
      const PoolNode pn = pool[xn];
      const int q = q0 + dd;
      PoolNode nn;
      nn.parent = dd - 1 > lo ? q - 1 : compact_index(w, M, j, dd - 1);
      nn.lpc = pn.lpc;
      nn.cht = pn.cht;
      out.node[q] = nn;
      out.up[q] = (dd & (kExpress - 1)) == 0 ? compact_index(w, M, j, dd - kExpress) : 0;  // stored on express levels only
      out.thi[q] = pool_thi[xn];
      xn = pn.parent;
      --dd;
    }
  }
  x.sync();
  if (x.uni(w.vars[CV_BAD]) != 0) return COMPACT_BAD_STATE;
  // the parked beam arrays: the entry's node, its parent, its express ancestor.  The dead-interior cache (via / viaanc / viach,
  // phase A2) is dropped instead: an entry that needs it walks once more and finds the same node under its new index.
  for (int j = tid; j < n; j += nt) {
    const int dj = compact_dep(arrays, K, j);
    b_node[j] = compact_index(w, M, j, dj);
    b_par[j] = dj == 0 ? -1 : compact_index(w, M, j, dj - 1);
    b_up[j] = dj == 0 ? 0 : compact_index(w, M, j, ((dj - 1) / kExpress) * kExpress);
    b_via[j] = -1;
    b_viaanc[j] = -1;
  }
  if (tid == 0) hdr[SH_POOL] = M;
  return COMPACT_OK;
}

// The new layout into a block (dst_pool, dst_pool_up as the kernels take them; dst_cap nodes): the stream's own, or a smaller one --
// then header and beam arrays (head_ints words) come along and the rest of the time steps' high parts start as zero, as in a
// fresh block.
template <class X>
CTC_HD void compact_write_back(X &x, int M, const CompactOut &src, const int *src_head, int *dst_head, size_t head_ints, PoolNode *dst_pool,
                               int *dst_pool_up, int dst_cap) {
  const size_t tid = (size_t)x.tid(), nt = (size_t)x.nt();
  int *d_node = reinterpret_cast<int *>(dst_pool), *d_up = dst_pool_up, *d_thi = dst_pool_up + dst_cap;
  const int *s_node = reinterpret_cast<const int *>(src.node);
  if (dst_head != src_head) {
    for (size_t i = tid; i < head_ints; i += nt) dst_head[i] = src_head[i];
    for (size_t i = (size_t)M + tid; i < (size_t)dst_cap; i += nt) d_thi[i] = 0;
  }
  for (size_t i = tid; i < (size_t)M * 3; i += nt) d_node[i] = s_node[i];
  for (size_t i = tid; i < (size_t)M; i += nt) { d_up[i] = src.up[i]; d_thi[i] = src.thi[i]; }
}

// what the host side asks the translation unit of the kernels for (stream_compact.hip).  Every per-stream array lives in ONE
// page-locked region the kernels read and write in place (ctl: its address as the device sees it).
struct CompactCtl {
  char *const *blocks;     // [B] the streams' blocks
  const int *pool_caps;    // [B] nodes their pools hold
  int *live;               // [B] out: nodes of the live set (count kernel; 0: no frames, -1: bad state)
  int *status;             // [B] out: COMPACT_* (gather kernel)
  char *const *dst;        // [B] where the new layout goes: the stream's block, or a smaller one
  const int *dst_caps;     // [B] nodes its pool holds
  const long long *scr;    // [B] offset (ints) of the stream's part of the scratch buffer
};
struct CompactLaunch {
  CompactCtl ctl;
  int *scratch;            // DEVICE: sum of compact_out_ints(live[b])
  long long pool_off;      // byte offset of the node pool inside a block
  int B, K;
};
size_t compact_lds_bytes(int K);
// queue ctc_stream_compact_count_kernel | ctc_stream_compact_gather_kernel + ctc_stream_compact_store_kernel on `stream`; return
// the hipError_t of the launch as an int
int launch_compact_count(const CompactLaunch &a, void *stream);
int launch_compact_move(const CompactLaunch &a, void *stream);
const void *compact_kernel_address(int which);  // 0 count, 1 gather, 2 store

}  // namespace ctccompact
