// stream_snapshot.h -- the image of a PARKED stream (beam_core.h StreamState / save_state) as a host byte string, and back: what
// ctcd_stream_save writes and ctcd_stream_restore reads.  A stream that has just been compacted (stream_compact.h) is its header
// words, its beam arrays and the M nodes of its live set in the canonical layout -- root at 0, entry 0's path, then every entry's own
// nodes, parents below children -- and nothing of that depends on the block's capacity or address, so the image is those words in a
// fixed order behind a header of its own:
//
//   [ SNAP_HDR_WORDS header | SH_WORDS header words | state_arrays(lm) * K beam arrays | 3 M node words | M express words | M high parts ]
//
// 32-bit little-endian words throughout; bytes = 4 * snapshot_words(K, lm, M).  The beam arrays hold entries 0 .. n - 1 as the
// compaction left them and zero behind (save_state writes the first n entries only: what lies behind them in a block is history).  A
// stream without frames is the root alone: zeroed header words and arrays, M = 1.
//
// snapshot_check() decides on the host, before anything is allocated or uploaded, whether an image may become a stream: the decode
// kernels follow the parked state's pool indices, its order array and (with a scorer) its table indices without a bounds check of their
// own, so an image passes only if every one of them is in range AND the nodes are exactly the layout its own depth and LCP arrays
// dictate -- the walks of finish(), the peek and phase A2 then end at the root after as many steps as the entry's depth says.
//
// The per-stream routines are written against an execution policy like stream_compact.h: the workgroup of stream_snapshot.hip on the
// GPU, a sequential one on the host (tests/native/snapshot_host.cpp).
#pragma once
#include <string.h>

#include <vector>

#include "stream_compact.h"

namespace ctcsnap {

using namespace ctcbeam;

constexpr uint32_t kSnapMagic = 0x53435443u;  // "CTCS"
constexpr int kSnapVersion = 1;
// the image's own header
enum { SN_MAGIC = 0, SN_VERSION, SN_TOTAL_WORDS, SN_BEAM, SN_LABELS, SN_SCORER_KIND, SN_FP_LO, SN_FP_HI, SN_FRAMES_LO, SN_FRAMES_HI,
       SN_COMMITTED_LO, SN_COMMITTED_HI, SN_NODES, SN_ARRAYS, SN_RESERVED0, SN_RESERVED1, SNAP_HDR_WORDS = 16 };
enum { SNAP_SCORER_NONE = 0, SNAP_SCORER_BUILTIN = 1 };

enum : int {
  SNAP_OK = 0,
  SNAP_TRUNCATED,    // fewer bytes than the fixed header, or than the header says
  SNAP_MAGIC,
  SNAP_VERSION,
  SNAP_SIZE,         // the byte count is not the one K / scorer kind / M give
  SNAP_BEAM,         // K against the restoring decoder
  SNAP_LABELS,       // V
  SNAP_SCORER_KIND,
  SNAP_FINGERPRINT,
  SNAP_HEADER,       // frames, n, pool count, select window
  SNAP_NODE,         // a node's parent
  SNAP_EXPRESS,      // a node's express word
  SNAP_BEAM_INDEX,   // a pool index in the beam arrays
  SNAP_FIN,          // the order array
  SNAP_DEPTH,        // dep / lcp
  SNAP_LABEL,        // a label word of the beam arrays
  SNAP_LM,           // an automaton state or dictionary word outside the scorer's tables
  SNAP_LAYOUT,       // the nodes are not the layout dep / lcp dictate
};
inline const char *snapshot_error_name(int code) {
  static const char *const names[] = {"ok", "truncated", "magic", "version", "size", "beam width", "label count", "scorer kind", "scorer fingerprint",
                                      "header word", "node parent", "express word", "beam pool index", "order array", "depth / lcp", "label word",
                                      "scorer table index", "node layout"};
  return code >= 0 && code < (int)(sizeof(names) / sizeof(names[0])) ? names[code] : "?";
}

CTC_HD size_t snapshot_head_words(int K, int lm) { return (size_t)SNAP_HDR_WORDS + SH_WORDS + (size_t)state_arrays(lm) * (size_t)K; }
CTC_HD size_t snapshot_words(int K, int lm, long long M) { return snapshot_head_words(K, lm) + ctccompact::compact_out_ints(M); }
CTC_HD size_t snapshot_bytes(int K, int lm, long long M) { return 4 * snapshot_words(K, lm, M); }
// where image b of a batch starts in one allocation: every image at a multiple of 16 bytes (128-bit accesses)
CTC_HD size_t snapshot_padded(size_t bytes) { return (bytes + 15) / 16 * 16; }

// what ctcd_snapshot_info reports (device-free)
struct SnapInfo {
  int version, beam, labels, scorer_kind, nodes, arrays;
  long long frames, committed;
  unsigned long long fingerprint;
  unsigned long long bytes;
};

// what the restoring decoder expects of an image
struct SnapExpect {
  int K, V, scorer_kind;
  unsigned long long fingerprint;
  // sizes of the scorer's tables (scorer_kind != 0): states, dictionary nodes, arc labels of a wide dictionary
  long long lm_states, lm_dict, lm_dict_lab;
  int lm_char_based, lm_dict_wide;
};
struct SnapError {
  int code;
  long long at;  // the word, entry or node the check failed at (-1: none)
};

// 64-bit FNV-1a over the scorer's tables as uploaded, and the scalars the kernels read beside them.  alpha / beta stay out:
// reset_params may change them mid-stream.  HS: lm_build.h HostScorer.
template <class HS>
inline unsigned long long scorer_fingerprint(const HS &h) {
  unsigned long long hsh = 1469598103934665603ull;
  auto mix = [&](const void *p, size_t bytes) {
    const unsigned char *c = (const unsigned char *)p;
    for (size_t i = 0; i < bytes; ++i) hsh = (hsh ^ c[i]) * 1099511628211ull;
  };
  auto vec = [&](const auto &v) {
    const unsigned long long n = v.size();
    mix(&n, 8);
    if (n) mix(v.data(), (size_t)n * sizeof(v[0]));
  };
  vec(h.uni_prob); vec(h.uni_state); vec(h.st_bo); vec(h.st_fail); vec(h.ng); vec(h.dict); vec(h.label_word); vec(h.dict_lab);
  const int sc[4] = {h.order, h.char_based ? 1 : 0, h.space_id, (int)h.dict.size()};
  mix(sc, sizeof(sc));
  return hsh ? hsh : 1;  // (0 is "no scorer")
}

namespace detail {
inline uint32_t rd(const void *blob, size_t word) {
  uint32_t v;
  memcpy(&v, (const char *)blob + word * 4, 4);
  return v;
}
inline long long rd64(const void *blob, size_t word) { return (long long)((unsigned long long)rd(blob, word) | ((unsigned long long)rd(blob, word + 1) << 32)); }
}  // namespace detail

// The fixed header alone.  SNAP_OK, or SNAP_TRUNCATED / SNAP_MAGIC / SNAP_VERSION / SNAP_SIZE.
inline int snapshot_info(const void *blob, size_t bytes, SnapInfo *out) {
  using detail::rd;
  if (!blob || bytes < (size_t)SNAP_HDR_WORDS * 4) return SNAP_TRUNCATED;
  if (rd(blob, SN_MAGIC) != kSnapMagic) return SNAP_MAGIC;
  if (rd(blob, SN_VERSION) != (uint32_t)kSnapVersion) return SNAP_VERSION;
  SnapInfo o;
  o.version = (int)rd(blob, SN_VERSION);
  o.beam = (int)rd(blob, SN_BEAM);
  o.labels = (int)rd(blob, SN_LABELS);
  o.scorer_kind = (int)rd(blob, SN_SCORER_KIND);
  o.nodes = (int)rd(blob, SN_NODES);
  o.arrays = (int)rd(blob, SN_ARRAYS);
  o.frames = detail::rd64(blob, SN_FRAMES_LO);
  o.committed = detail::rd64(blob, SN_COMMITTED_LO);
  o.fingerprint = (unsigned long long)detail::rd64(blob, SN_FP_LO);
  if (o.beam < 1 || o.beam > kMaxBeam || o.nodes < 1 || (o.scorer_kind != SNAP_SCORER_NONE && o.scorer_kind != SNAP_SCORER_BUILTIN)) return SNAP_SIZE;
  if (o.arrays != state_arrays(o.scorer_kind)) return SNAP_SIZE;
  const size_t want = snapshot_bytes(o.beam, o.scorer_kind, o.nodes);
  o.bytes = want;
  if (rd(blob, SN_TOTAL_WORDS) != (uint32_t)(want / 4) || rd(blob, SN_RESERVED0) != 0 || rd(blob, SN_RESERVED1) != 0) return SNAP_SIZE;
  if (bytes < want) return SNAP_TRUNCATED;
  if (bytes != want) return SNAP_SIZE;
  if (out) *out = o;
  return SNAP_OK;
}

// Everything a later kernel follows.  `blob` need not be aligned.  Returns SNAP_OK or the first check that fails (err, if not null:
// the check and where).
inline int snapshot_check(const void *blob, size_t bytes, const SnapExpect &e, SnapError *err = nullptr) {
  using detail::rd;
  namespace cc = ctccompact;
  auto fail = [&](int code, long long at) { if (err) { err->code = code; err->at = at; } return code; };
  if (err) { err->code = SNAP_OK; err->at = -1; }
  SnapInfo in;
  const int hc = snapshot_info(blob, bytes, &in);
  if (hc != SNAP_OK) return fail(hc, -1);
  if (in.beam != e.K) return fail(SNAP_BEAM, SN_BEAM);
  if (in.labels != e.V) return fail(SNAP_LABELS, SN_LABELS);
  if (in.scorer_kind != e.scorer_kind) return fail(SNAP_SCORER_KIND, SN_SCORER_KIND);
  if (in.fingerprint != (e.scorer_kind ? e.fingerprint : 0ull)) return fail(SNAP_FINGERPRINT, SN_FP_LO);
  const int K = in.beam, M = in.nodes, lm = in.scorer_kind;
  const size_t o_hdr = SNAP_HDR_WORDS, o_arr = o_hdr + SH_WORDS, o_node = snapshot_head_words(K, lm), o_up = o_node + (size_t)M * 3, o_thi = o_up + (size_t)M;
  (void)o_thi;
  auto hdr = [&](int i) { return (int)rd(blob, o_hdr + (size_t)i); };
  auto arr = [&](int a, int j) { return (int)rd(blob, o_arr + (size_t)a * K + (size_t)j); };
  const long long frames = in.frames;
  if (frames < 0 || frames > 0x7fffffffLL || in.committed < 0 || hdr(SH_FRAMES) != (int)frames) return fail(SNAP_HEADER, SH_FRAMES);
  // node 0 is the root; every other node has its parent below it and its express word at or below it
  if ((int)rd(blob, o_node) != -1) return fail(SNAP_NODE, 0);
  if (rd(blob, o_up) != 0) return fail(SNAP_EXPRESS, 0);
  for (int i = 1; i < M; ++i) {
    const int p = (int)rd(blob, o_node + (size_t)i * 3), u = (int)rd(blob, o_up + (size_t)i);
    if (p < 0 || p >= i) return fail(SNAP_NODE, i);
    if (u < 0 || u > i) return fail(SNAP_EXPRESS, i);
  }
  if (frames == 0) {  // a stream without frames: the root alone, a zeroed head
    if (M != 1 || in.committed != 0) return fail(SNAP_HEADER, SH_POOL);
    for (size_t i = o_hdr; i < o_node; ++i)
      if (rd(blob, i) != 0 && i != o_hdr + SH_POOL) return fail(SNAP_HEADER, (long long)(i - o_hdr));
    if (hdr(SH_POOL) != 1) return fail(SNAP_HEADER, SH_POOL);
    return SNAP_OK;
  }
  const int n = hdr(SH_N);
  if (n < 1 || n > K) return fail(SNAP_HEADER, SH_N);
  if (hdr(SH_POOL) != M) return fail(SNAP_HEADER, SH_POOL);
  if (hdr(SH_WLOG) < kBinsLog || hdr(SH_WLOG) > 32) return fail(SNAP_HEADER, SH_WLOG);  // (the select shifts by it)
  const int idx_arrays[5] = {cc::CA_NODE, cc::CA_PAR, cc::CA_VIA, cc::CA_VIAANC, cc::CA_UP};
  const int A = state_arrays(lm);
  for (int j = 0; j < n; ++j) {
    for (int a = 0; a < 5; ++a) {
      const int v = arr(idx_arrays[a], j);
      if (v < -1 || v >= M) return fail(SNAP_BEAM_INDEX, (long long)idx_arrays[a] * K + j);
    }
    if (arr(cc::CA_NODE, j) < 0 || arr(cc::CA_UP, j) < 0) return fail(SNAP_BEAM_INDEX, (long long)cc::CA_NODE * K + j);
    const int f = arr(13, j);
    if (f < 0 || f >= n) return fail(SNAP_FIN, j);
    const int d = arr(cc::CA_DEP, j), l = arr(cc::CA_LCP, j);
    if (d < -1 || d > frames || l < -1 || l > frames) return fail(SNAP_DEPTH, j);
    const int ch = arr(2, j), vch = arr(7, j);
    if (ch < -1 || ch >= e.V || vch < -1 || vch >= e.V) return fail(SNAP_LABEL, j);
    if (lm) {
      const long long st = (uint32_t)arr(kStateArrays + 0, j), sp = (uint32_t)arr(kStateArrays + 10, j);
      if (st >= e.lm_states || sp >= e.lm_states) return fail(SNAP_LM, j);
      if (!e.lm_char_based) {
        const long long dn = (uint32_t)arr(kStateArrays + 4, j), lo = (uint32_t)arr(kStateArrays + 5, j), hi = (uint32_t)arr(kStateArrays + 6, j);
        const int fc = arr(kStateArrays + 7, j);
        if (dn >= e.lm_dict) return fail(SNAP_LM, j);
        if (fc < -1) return fail(SNAP_LM, j);
        if (fc >= 0) {  // (-1: pending, resolved from the node's own record)
          const long long kids = e.lm_dict_wide ? hi : (long long)__builtin_popcount((uint32_t)lo) + __builtin_popcount((uint32_t)hi);
          if ((long long)fc + kids > e.lm_dict) return fail(SNAP_LM, j);
          if (e.lm_dict_wide && lo + hi > e.lm_dict_lab) return fail(SNAP_LM, j);
        }
      }
    }
  }
  // entries behind n: zero, as save writes them
  for (int a = 0; a < A; ++a)
    for (int j = n; j < K; ++j)
      if (arr(a, j) != 0) return fail(SNAP_BEAM_INDEX, (long long)a * K + j);
  // the layout: with lo[j] = lcp[j] clamped into [0, dep[j]] (entry 0: 0) entry j owns dep[j] - lo[j] consecutive nodes, and shares
  // the first lo[j] labels of its path with its predecessor -- which therefore is at least that deep
  std::vector<int> lo((size_t)n), base((size_t)n), blkmin((size_t)n / cc::kCompactBlk + 1, kIntMax);
  long long total = 1;
  for (int j = 0; j < n; ++j) {
    int d = arr(cc::CA_DEP, j);
    d = d < 0 ? 0 : d;
    int l = j == 0 ? 0 : arr(cc::CA_LCP, j);
    l = l < 0 ? 0 : (l > d ? d : l);
    if (j > 0) {
      int dp = arr(cc::CA_DEP, j - 1);
      dp = dp < 0 ? 0 : dp;
      if (l > dp) return fail(SNAP_DEPTH, j);
    }
    lo[j] = l;
    base[j] = (int)total;
    total += d - l;
    if (total > M) return fail(SNAP_LAYOUT, j);
    int &bm = blkmin[(size_t)j / cc::kCompactBlk];
    bm = l < bm ? l : bm;
  }
  if (total != M) return fail(SNAP_LAYOUT, n);
  cc::CompactWork w;
  w.base = base.data(); w.lo = lo.data(); w.blkmin = blkmin.data(); w.part = nullptr; w.pmax = nullptr; w.vars = nullptr;
  for (int j = 0; j < n; ++j) {
    int d = arr(cc::CA_DEP, j);
    d = d < 0 ? 0 : d;
    if (arr(cc::CA_NODE, j) != cc::compact_index(w, M, j, d)) return fail(SNAP_LAYOUT, j);
    if (arr(cc::CA_PAR, j) != (d == 0 ? -1 : cc::compact_index(w, M, j, d - 1))) return fail(SNAP_LAYOUT, j);
    if (arr(cc::CA_UP, j) != (d == 0 ? 0 : cc::compact_index(w, M, j, ((d - 1) / kExpress) * kExpress))) return fail(SNAP_LAYOUT, j);
    for (int dd = lo[j] + 1; dd <= d; ++dd) {
      const int q = base[j] + dd - lo[j] - 1;
      const int want_p = dd - 1 > lo[j] ? q - 1 : cc::compact_index(w, M, j, dd - 1);
      const int want_u = (dd & (kExpress - 1)) == 0 ? cc::compact_index(w, M, j, dd - kExpress) : 0;
      if ((int)rd(blob, o_node + (size_t)q * 3) != want_p) return fail(SNAP_NODE, q);
      if ((int)rd(blob, o_up + (size_t)q) != want_u) return fail(SNAP_EXPRESS, q);
    }
  }
  return SNAP_OK;
}

// ---- the per-stream routines ----------------------------------------------------------------------------------------------------
constexpr int kSnapThreads = 256;

// n words from src to dst by the threads of X: four at a time where both are 16-byte aligned at the same word
template <class X>
CTC_HD void snap_copy(X &x, int *dst, const int *src, size_t n) {
  const size_t tid = (size_t)x.tid(), nt = (size_t)x.nt();
  const size_t da = ((size_t)(uintptr_t)dst >> 2) & 3, sa = ((size_t)(uintptr_t)src >> 2) & 3;
  if (da != sa || n < 8) {
    for (size_t i = tid; i < n; i += nt) dst[i] = src[i];
    return;
  }
  const size_t head = (4 - da) & 3, quads = (n - head) / 4, tail0 = head + quads * 4;
  for (size_t i = tid; i < head; i += nt) dst[i] = src[i];
  Int4v *d4 = reinterpret_cast<Int4v *>(dst + head);
  const Int4v *s4 = reinterpret_cast<const Int4v *>(src + head);
  for (size_t i = tid; i < quads; i += nt) d4[i] = s4[i];
  for (size_t i = tail0 + tid; i < n; i += nt) dst[i] = src[i];
}

// the facts of a stream the host knows and the image carries
struct SnapMeta {
  long long frames, committed;
  unsigned long long fingerprint;
  int V, scorer_kind;
};

// One stream's image from its block, which a compaction has just left in the canonical layout (M nodes: what it reported; a stream
// without frames: 1).  img: snapshot_words(K, lm, M) words.  hdr / arrays / pool / pool_up as the kernels take them.
template <class X>
CTC_HD void snapshot_export(X &x, int K, int M, const SnapMeta &m, const int *hdr, const int *arrays, const PoolNode *pool, const int *pool_up,
                            int pool_cap, int *img) {
  const size_t tid = (size_t)x.tid(), nt = (size_t)x.nt();
  const int lm = m.scorer_kind != SNAP_SCORER_NONE ? 1 : 0, A = state_arrays(lm);
  const size_t head = snapshot_head_words(K, lm);
  if (tid == 0) {
    img[SN_MAGIC] = (int)kSnapMagic; img[SN_VERSION] = kSnapVersion; img[SN_TOTAL_WORDS] = (int)snapshot_words(K, lm, M);
    img[SN_BEAM] = K; img[SN_LABELS] = m.V; img[SN_SCORER_KIND] = m.scorer_kind;
    img[SN_FP_LO] = (int)(uint32_t)m.fingerprint; img[SN_FP_HI] = (int)(uint32_t)(m.fingerprint >> 32);
    img[SN_FRAMES_LO] = (int)(uint32_t)m.frames; img[SN_FRAMES_HI] = (int)(uint32_t)((unsigned long long)m.frames >> 32);
    img[SN_COMMITTED_LO] = (int)(uint32_t)m.committed; img[SN_COMMITTED_HI] = (int)(uint32_t)((unsigned long long)m.committed >> 32);
    img[SN_NODES] = M; img[SN_ARRAYS] = A; img[SN_RESERVED0] = 0; img[SN_RESERVED1] = 0;
  }
  int *o_hdr = img + SNAP_HDR_WORDS, *o_arr = o_hdr + SH_WORDS, *o_node = img + head;
  if (m.frames <= 0) {  // nothing fed: the root alone (what the block holds is zeroed memory, or a beam no frame has touched)
    for (size_t i = tid; i < (size_t)SH_WORDS + (size_t)A * K; i += nt) o_hdr[i] = i == (size_t)SH_POOL ? 1 : 0;
    if (tid == 0) { o_node[0] = -1; o_node[1] = 0; o_node[2] = 0xFFFF; o_node[3] = 0; o_node[4] = 0; }
    return;
  }
  for (size_t i = tid; i < (size_t)SH_WORDS; i += nt) o_hdr[i] = i < 10 ? hdr[i] : 0;  // (the reserved words travel as zero)
  int n = hdr[SH_N];
  n = n < 0 ? 0 : (n > K ? K : n);
  if (n == K) {
    snap_copy(x, o_arr, arrays, (size_t)A * K);
  } else {
    for (size_t i = tid; i < (size_t)A * K; i += nt) o_arr[i] = (int)(i % (size_t)K) < n ? arrays[i] : 0;
  }
  snap_copy(x, o_node, reinterpret_cast<const int *>(pool), (size_t)M * 3);
  snap_copy(x, o_node + (size_t)M * 3, pool_up, (size_t)M);
  snap_copy(x, o_node + (size_t)M * 4, pool_up + pool_cap, (size_t)M);
}

// The inverse, into a fresh block of dst_cap >= M nodes (head_ints: the words of the block in front of its pool): header words and
// beam arrays, the rest of the head zero, the nodes with their express words and high parts, the rest of the high parts zero -- the
// smaller-block route of compact_write_back.  img has passed snapshot_check.
template <class X>
CTC_HD void snapshot_import(X &x, const int *img, int *dst_head, size_t head_ints, PoolNode *dst_pool, int *dst_pool_up, int dst_cap) {
  const size_t tid = (size_t)x.tid(), nt = (size_t)x.nt();
  const int K = img[SN_BEAM], M = img[SN_NODES], lm = img[SN_SCORER_KIND] != SNAP_SCORER_NONE ? 1 : 0;
  const size_t live = (size_t)SH_WORDS + (size_t)state_arrays(lm) * K;
  if (img[SN_FRAMES_LO] == 0 && img[SN_FRAMES_HI] == 0) {  // a fresh stream: a zeroed head (the first chunk initialises the beam), zeroed high parts
    for (size_t i = tid; i < head_ints; i += nt) dst_head[i] = 0;
    for (size_t i = tid; i < (size_t)dst_cap; i += nt) dst_pool_up[(size_t)dst_cap + i] = 0;
    return;
  }
  for (size_t i = live + tid; i < head_ints; i += nt) dst_head[i] = 0;
  ctccompact::compact_write_back(x, M, ctccompact::compact_out_at(const_cast<int *>(img) + snapshot_head_words(K, lm), M), img + SNAP_HDR_WORDS, dst_head,
                                 live, dst_pool, dst_pool_up, dst_cap);
}

// what the host side asks the translation unit of the kernels for (stream_snapshot.hip).  The per-stream arrays live in one
// page-locked region the kernels read in place.
struct SnapCtl {
  char *const *blocks;     // [B] the streams' blocks
  const int *pool_caps;    // [B] nodes their pools hold
  const int *nodes;        // [B] export: M of every stream
  const long long *off;    // [B] offset (ints) of the stream's image in the staging buffer
  const SnapMeta *meta;    // [B] export
};
struct SnapLaunch {
  SnapCtl ctl;
  int *staging;            // DEVICE: the images, each at its offset
  long long pool_off;      // byte offset of the node pool inside a block
  int B, K;
};
// queue ctc_stream_export_kernel / ctc_stream_import_kernel on `stream`; return the hipError_t of the launch as an int
int launch_snapshot_export(const SnapLaunch &a, void *stream);
int launch_snapshot_import(const SnapLaunch &a, void *stream);
const void *snapshot_kernel_address(int which);  // 0 export, 1 import

}  // namespace ctcsnap
