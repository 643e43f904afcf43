// stream_commit.h -- commit of a PARKED scorer-free stream's final labels (beam_core.h StreamState / save_state): the labels every
// current beam entry shares are final (stream_peek.h: the common prefix only grows, its labels and time steps never change again),
// so all of them but the last are handed to the caller once and their nodes -- the trunk of the trie -- dropped with the dead
// nodes: the node of depth D = stable_len - 1 on the common path becomes the root, and the stream goes on as one whose root has
// dropped out of the beam.  With D == 0 this is stream_compact.h's compaction, byte for byte.
//
// Why no decode kernel needs to know: without a scorer beam_core.h uses a depth only in differences (phase A1 / A2's hops, the
// lcp[j + 1] >= dep[j] tests, finish()'s segments (lcp[j], dep[j]], the walks of the peek and of the compaction), a back-trace stops
// by depth count and not at parent == -1, and every pool access starts from a beam entry -- no entry is shallower than the common
// prefix.  Reducing dep[] and lcp[1..] by D and laying the live set out below the new root is a state the kernels meet anyway.
// Absolute depth appears with a scorer only (finish(): ap - dep * beta, dep == 0 = the empty sentence; stream_peek.h
// lm_final_scores): streams with a scorer are refused on the host side.
//
// The layout is stream_compact.h's with every depth reduced by D: entry 0 owns its nodes of depth D + 1 .. dep[0], every other entry
// what it owned (lcp[j] >= stable_len > D for j >= 1).  compact_plan() lays entry 0's whole path out first, by increasing depth --
// its node of depth e at index e -- so the new index of a live node is its index in that layout minus D, the new root at 0, and
// compact_plan / compact_index are used as they are.  The express pointers are rewritten from the new layout (new depth = 0 mod
// kExpress), wherever D falls; the old ones are only read, in old coordinates, to reach the segments.
//
// The per-stream routines are written against an execution policy like stream_compact.h: the workgroup of stream_commit.hip on the
// GPU, a sequential one on the host (tests/native/commit_host.cpp).
#pragma once
#include "stream_compact.h"

namespace ctccommit {

using namespace ctccompact;

struct CommitPlan {
  CompactPlan cp;  // the compaction's plan of the state as it is (old coordinates; cp.M: 0 = no frames, -1 = bad state)
  int drop;        // D: labels committed now = nodes of the trunk that leave (0: a plain compaction)
  int M;           // nodes the stream keeps, new root included: cp.M - D (cp.M <= 0: cp.M)
};

// The layout and the drop.  X as in compact_plan.  Identical in every thread.
template <class X>
CTC_HD CommitPlan commit_plan(X &x, const CompactWork &w, int K, const int *hdr, const int *arrays, int pool_cap) {
  CommitPlan pl;
  pl.cp = compact_plan(x, w, K, hdr, arrays, pool_cap);
  pl.drop = 0;
  pl.M = pl.cp.M;
  if (pl.cp.M <= 0) return pl;
  const int tid = x.tid(), nt = x.nt(), n = pl.cp.n;
  // stable_len = min(lcp[1 .. n-1]), dep[0] for a single entry (peek_stream) -- on the clamped values the layout was made from
  // (lo[j] <= dep[j]), and never deeper than entry 0: the trunk is read along entry 0's path
  int m = kIntMax;
  for (int j = 1 + tid; j < n; j += nt) m = w.lo[j] < m ? w.lo[j] : m;
  w.pmax[tid] = m;  // (compact_plan is done with it: its last barrier is behind us)
  x.sync();
  for (int t = 0; t < nt; ++t) m = w.pmax[t] < m ? w.pmax[t] : m;
  const int d0 = compact_dep(arrays, K, 0);
  const int s = m < d0 ? m : d0;
  pl.drop = s > 1 ? s - 1 : 0;
  pl.M = pl.cp.M - pl.drop;
  x.sync();  // (pmax may be written again)
  return pl;
}

// New index of the node at OLD depth e >= D of entry j's path (e <= D: the new root).
CTC_HD int commit_index(const CompactWork &w, const CommitPlan &pl, int j, int e) {
  if (e <= pl.drop) return 0;
  const int q = compact_index(w, pl.cp.M, j, e) - pl.drop;
  return q > 0 ? q : 0;  // (outside the layout: a state no save_state wrote; the index stays inside the pool)
}

// Gathers the live set of one stream below its new root into `out` (pl.M nodes), reads the trunk -- labels and ABSOLUTE time steps
// of the old depths 1 .. D -- into c_tok / c_ts [D], then rewrites the parked beam arrays IN the block: the pool indices as
// compact_gather does, dep[] and lcp[1..] reduced by D, the pool count.  The old pool is only read.  Tasks are compact_gather's
// (entry, segment of kExpress hops) pairs, one thread each; entry 0's reach down to the old root, so that the trunk is read back
// segment by segment over the express pointers like every other path and never as one chain of D dependent loads.
// Returns COMPACT_OK or COMPACT_BAD_STATE (identical in every thread; bad: a walk left the pool -- the block is unchanged).
template <class X>
CTC_HD int commit_gather(X &x, const CompactWork &w, const CommitPlan &pl, int K, int *hdr, int *arrays, const PoolNode *pool,
                         const int *pool_up, int pool_cap, const CompactOut &out, int32_t *c_tok, int32_t *c_ts) {
  const int tid = x.tid(), nt = x.nt();
  const int n = pl.cp.n, D = pl.drop;
  const int *pool_thi = pool_up + pool_cap;
  const bool long_t = x.uni(hdr[SH_FRAMES]) > 65536;  // (frame numbers 0 .. 65535 fit the node's 16 bits: peek_stream)
  int *b_node = arrays + (size_t)CA_NODE * K, *b_par = arrays + (size_t)CA_PAR * K, *b_up = arrays + (size_t)CA_UP * K;
  int *b_via = arrays + (size_t)CA_VIA * K, *b_viaanc = arrays + (size_t)CA_VIAANC * K;
  int *b_dep = arrays + (size_t)CA_DEP * K, *b_lcp = arrays + (size_t)CA_LCP * K;
  if (tid == 0) {
    if (pool_cap <= 0) {
      w.vars[CV_BAD] = 1;
    } else if (D == 0) {  // the root stays
      PoolNode r = pool[0];
      r.parent = -1;
      out.node[0] = r; out.up[0] = 0; out.thi[0] = pool_thi[0];
    }
  }
  const long long nseg = (long long)pl.cp.maxdep / kExpress + 1;
  for (long long idx = tid; idx < nseg * n; idx += nt) {
    const int i = (int)(idx / n), j = (int)(idx - (long long)i * n);
    const int dj = compact_dep(arrays, K, j);
    const int lo = j == 0 ? 0 : w.lo[j];       // what the walk stops at: entry 0's goes through the trunk
    const int own = j == 0 ? D : lo;           // the depth below which the entry owns no node of the new layout
    const int top = ((dj - 1) / kExpress) * kExpress;  // OLD depth of the first express ancestor
    if (dj <= lo || i > top / kExpress) continue;
    int dd = i == 0 ? dj : top - (i - 1) * kExpress;
    int stop = i == 0 ? top : dd - kExpress;
    if (dd <= lo) continue;
    stop = stop < lo ? lo : stop;
    int xn;
    if (i == 0) {
      xn = b_node[j];
    } else {
      xn = b_up[j];
      for (int h = 1; h < i && (unsigned)xn < (unsigned)pool_cap; ++h) xn = pool_up[xn];
    }
    const int q0 = w.base[j] - w.lo[j] - 1 - D;  // entry j's node of OLD depth e > own goes to q0 + e (entry 0: e - D)
    while (dd > stop) {
      if ((unsigned)xn >= (unsigned)pool_cap) { w.vars[CV_BAD] = 1; break; }  // (a node index outside the pool is not followed)
      const PoolNode pn = pool[xn];
      if (dd > own) {
        const int q = q0 + dd;
        PoolNode nn;
        nn.parent = dd - 1 > own ? q - 1 : commit_index(w, pl, j, dd - 1);
        nn.lpc = pn.lpc;
        nn.cht = pn.cht;
        out.node[q] = nn;
        out.up[q] = ((dd - D) & (kExpress - 1)) == 0 ? commit_index(w, pl, j, dd - kExpress) : 0;  // on the NEW express levels only
        out.thi[q] = pool_thi[xn];
      } else {  // (entry 0, depths 1 .. D: the trunk)
        c_tok[dd - 1] = pn.ch();
        c_ts[dd - 1] = (int)(pn.cht >> 16) | (long_t ? pool_thi[xn] << 16 : 0);
        if (dd == D) {  // its last node: the new root.  Its own lpc / cht / thi stay -- no back-trace reaches depth 0
          PoolNode r = pn;
          r.parent = -1;
          out.node[0] = r; out.up[0] = 0; out.thi[0] = pool_thi[xn];
        }
      }
      xn = pn.parent;
      --dd;
    }
  }
  x.sync();
  if (x.uni(w.vars[CV_BAD]) != 0) return COMPACT_BAD_STATE;
  for (int j = tid; j < n; j += nt) {
    const int dj = compact_dep(arrays, K, j);
    const int nd = dj - D;  // (>= 1 whenever D > 0)
    b_node[j] = commit_index(w, pl, j, dj);
    b_par[j] = nd <= 0 ? -1 : commit_index(w, pl, j, dj - 1);
    b_up[j] = nd <= 0 ? 0 : commit_index(w, pl, j, D + ((nd - 1) / kExpress) * kExpress);
    b_via[j] = -1;
    b_viaanc[j] = -1;
    if (D > 0) {
      b_dep[j] = nd;
      if (j > 0) b_lcp[j] -= D;  // (entry 0 keeps its -1)
    }
  }
  if (tid == 0) hdr[SH_POOL] = pl.M;
  return COMPACT_OK;
}

// what the host side asks the translation unit of the kernels for (stream_commit.hip).  The per-stream arrays live in one
// page-locked region as the compaction's do (CompactCtl: live[b] = the compaction's count of the state as it is).
struct CommitCtl {
  CompactCtl c;
  int *drop;             // [B] out: labels stream b commits now (count kernel)
  const long long *lab;  // [B] offset (ints) of the stream's committed labels in the scratch buffer: drop[b] tokens, then drop[b] time steps
};
struct CommitLaunch {
  CommitCtl ctl;
  int *scratch;          // DEVICE: sum of compact_out_ints(live[b] - drop[b]), then the labels
  long long pool_off;    // byte offset of the node pool inside a block
  int B, K;
};
// queue ctc_stream_commit_count_kernel | ctc_stream_commit_gather_kernel + ctc_stream_commit_store_kernel on `stream`; return the
// hipError_t of the launch as an int
int launch_commit_count(const CommitLaunch &a, void *stream);
int launch_commit_move(const CommitLaunch &a, void *stream);
const void *commit_kernel_address(int which);  // 0 count, 1 gather, 2 store

}  // namespace ctccommit
