// nbest.h -- rows 0 .. n-1 alone out of the compact result form (beam_core.h OutRefs::c_*, include/ctcdecode_amd.h "n-best
// results"): output / timesteps [B, n, T], scores / out_lens [B, n], defined everywhere -- label positions at or beyond a row's
// length are 0, a row without a result has length 0, score 0 and zero labels.
//
// The records of one item: c_hdr = {#results, #labels, first label's index in c_labels, 0}; entry j of c_ent (trie order) =
// {result row, lcp = #labels shared with entry j-1, length, index of its own labels [lcp, length) in c_labels}.  Label q of entry j
// is held by the nearest entry o <= j with lcp[o] <= q.  Walking back from j with the running minimum m of lcp over (o, j], entry o
// holds the positions [lcp[o], min(m, hi)) -- the SEGMENTS of row j, found in descending order, each ending where the one before it
// starts.  A selected row's segments are mostly held by entries that are not selected; finding them reads entry tables only, never a
// label of a row that is not asked for.
//
// Every index is checked before it is followed (entry_ok / segment_ok below): a malformed record zeroes the rows that would have
// drawn labels from it and raises the item's status word to NBEST_BAD_RECORD; it never becomes an out-of-range access.
//
// All of the index arithmetic is CTC_HD code: the kernel of nbest.hip and the host twin (tests/native/nbest_host.cpp) compile the same
// routines.  expand_item_nbest_host is the product's host expansion (ctcd_beam_decode_to_host_nbest): one row buffer over the entries
// in trie order, as expand_item_host keeps it, streamed out for the rows below n only.  rows_by_segments_host is the kernel's method
// run sequentially, for the host tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "compact_results.h"

#ifndef CTC_HD
#if defined(__HIPCC__)
#define CTC_HD __host__ __device__ __forceinline__
#else
#define CTC_HD inline
#endif
#endif

namespace ctcnbest {

constexpr int kNbestMaxK = 4096;       // entries whose tables fit LDS (ctcd_expand_compact has the same limit)
constexpr int kNbestMaxThreads = 256;  // one wave per selected row, at most four of them at a time
constexpr int kNoEntry = 0x7fffffff;   // sel[p]: no entry has result row p
enum : int { NBEST_BAD_RECORD = 7 };   // the status word of an item with a malformed record (beam_core.h ST_* end at 6)

// workgroup size: a wave per selected row -- n = 1 writes 8 bytes x T with one wave, not with sixteen
CTC_HD int nbest_threads(int n) { return n <= 1 ? 64 : (n == 2 ? 128 : (n == 3 ? 192 : kNbestMaxThreads)); }
// LDS: lcp / dep / off [K], sel [n], and per wave the segment list (entry indices, 16 bits each: K <= 4096)
CTC_HD size_t seg_stride(int K) { return ((size_t)K + 1) / 2 * 2; }
CTC_HD size_t nbest_lds_bytes(int K, int n, int threads) { return ((size_t)3 * K + (size_t)n) * 4 + (size_t)(threads / 64) * seg_stride(K) * 2; }
// the 16-byte store path: rows of whole 16-byte words on both tensors
CTC_HD bool nbest_vec16(int T, uintptr_t tok, uintptr_t ts) { return T % 4 == 0 && tok % 16 == 0 && ts % 16 == 0; }

CTC_HD int clamp_count(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// An item's header: #results in [0, K] and its labels [first, first + total) inside the label buffer, or the item is malformed
struct ItemView {
  int nres;
  uint32_t first, total;
  bool ok;
};
CTC_HD ItemView item_view(const int32_t *hdr, int b, int K, unsigned long long n_labels) {
  const int32_t *h = hdr + (size_t)b * 4;
  ItemView v;
  v.first = (uint32_t)h[2];
  v.total = (uint32_t)h[1];
  v.ok = h[0] >= 0 && h[0] <= K && (unsigned long long)v.first + v.total <= n_labels;
  v.nres = v.ok ? h[0] : 0;
  return v;
}

// entry j as the walk uses it: lcp in [0, T] whatever the record says (entry 0 shares nothing), length -1 when the entry is malformed
struct Entry {
  int row, lcp, dep;
  uint32_t off;
  bool ok;
};
CTC_HD Entry entry_view(const int32_t *e, int j, int K, int T, const ItemView &it) {
  Entry r;
  r.row = e[0];
  const int lcp = j == 0 ? 0 : e[1], dep = e[2];
  r.off = (uint32_t)e[3];
  const uint32_t rel = r.off - it.first;  // (wraps for an offset below the item's first label: then > total)
  r.ok = (unsigned)r.row < (unsigned)K && lcp >= 0 && lcp <= dep && dep <= T && rel <= it.total && (uint32_t)(dep - lcp) <= it.total - rel;
  r.lcp = clamp_count(lcp, T);
  r.dep = r.ok ? dep : -1;
  return r;
}

// segment [lcp[o], hi) of entry o: held by a well-formed entry that is long enough (its length -1 when malformed: never)
CTC_HD bool segment_ok(int dep_o, int hi) { return dep_o >= hi; }

// the segment of position q: the first s with lcp[seg[s]] <= q (the starts descend; the last segment starts at 0)
template <typename SegT> CTC_HD int seg_find(const SegT *seg, const int *lcp, int nseg, int q) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lcp[seg[mid]] <= q) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
// ... and of the position after one whose segment is s
template <typename SegT> CTC_HD int seg_next(const SegT *seg, const int *lcp, int s, int q) {
  while (s > 0 && lcp[seg[s - 1]] <= q) --s;
  return s;
}
// where label q of a row lies in c_labels, given its segment's entry o
CTC_HD uint32_t label_index(uint32_t off_o, int lcp_o, int q) { return off_o + (uint32_t)(q - lcp_o); }

// ---- the product's host expansion ------------------------------------------------------------------------------------------------
// Item b: one row buffer over the entries in trie order; every entry updates it, the rows below n are streamed out (tok / ts:
// [B, n, T]).  `valid` = the leading positions of the buffer that well-formed entries wrote.  row_ok (n bytes, or NULL): 1 for the
// rows that have a well-formed result.  Returns 0, or NBEST_BAD_RECORD.
inline int expand_item_nbest_host(const int32_t *hdr, const int32_t *ent, const uint32_t *rag, unsigned long long n_labels, int b, int K, int T, int n,
                                  int32_t *tok, int32_t *ts, unsigned char *row_ok) {
  const ItemView it = item_view(hdr, b, K, n_labels);
  int status = it.ok ? 0 : NBEST_BAD_RECORD;
  int32_t *tk0 = tok + (size_t)b * n * T, *ts0 = ts + (size_t)b * n * T;
  std::vector<unsigned char> used((size_t)n, 0);
  std::vector<int32_t> buf((size_t)2 * T + 8, 0);
  int32_t *bt = buf.data(), *bs = buf.data() + T + 4;
  int valid = 0;
  for (int j = 0; j < it.nres; ++j) {
    const Entry e = entry_view(ent + ((size_t)b * K + j) * 4, j, K, T, it);
    bool good = e.ok && e.lcp <= valid;
    if (!e.ok) status = NBEST_BAD_RECORD;
    if (e.ok) {
      const uint32_t *seg = rag + e.off;
      for (int q = e.lcp; q < e.dep; ++q) {
        const uint32_t v = seg[q - e.lcp];
        bt[q] = (int32_t)(v & 0xFFFFu);
        bs[q] = (int32_t)(v >> 16);
      }
      if (good) valid = e.dep;
    } else if (e.lcp < valid) {
      valid = e.lcp;
    }
    if ((unsigned)e.row >= (unsigned)n) continue;
    if (used[(size_t)e.row]) {  // a second entry for a row: the first one stays
      status = NBEST_BAD_RECORD;
      continue;
    }
    used[(size_t)e.row] = good ? 1 : 2;
    if (!good) {
      status = NBEST_BAD_RECORD;
      continue;
    }
    ctcbeam::stream_row(tk0 + (size_t)e.row * T, bt, e.dep, T);
    ctcbeam::stream_row(ts0 + (size_t)e.row * T, bs, e.dep, T);
  }
  for (int p = 0; p < n; ++p) {
    if (row_ok) row_ok[p] = used[(size_t)p] == 1;
    if (used[(size_t)p] != 1) {
      ctcbeam::stream_row(tk0 + (size_t)p * T, bt, 0, T);
      ctcbeam::stream_row(ts0 + (size_t)p * T, bs, 0, T);
    }
  }
#if defined(__x86_64__)
  _mm_sfence();
#endif
  return status;
}

// ---- the kernel's method, sequentially (host tests) ------------------------------------------------------------------------------
// Stages the tables as the kernel does, selects the first entry of every row below n, walks back from each for its segments and
// writes the row position by position through seg_find / seg_next / label_index.  Same outputs and return value as above.
inline int rows_by_segments_host(const int32_t *hdr, const int32_t *ent, const uint32_t *rag, unsigned long long n_labels, int b, int K, int T, int n,
                                 int32_t *tok, int32_t *ts, unsigned char *row_ok) {
  const ItemView it = item_view(hdr, b, K, n_labels);
  int status = it.ok ? 0 : NBEST_BAD_RECORD;
  std::vector<int> lcp((size_t)K + 1), dep((size_t)K + 1), sel((size_t)n, kNoEntry);
  std::vector<uint32_t> off((size_t)K + 1);
  std::vector<uint16_t> seg(seg_stride(K));
  for (int j = 0; j < it.nres; ++j) {
    const Entry e = entry_view(ent + ((size_t)b * K + j) * 4, j, K, T, it);
    lcp[(size_t)j] = e.lcp; dep[(size_t)j] = e.dep; off[(size_t)j] = e.off;
    if (!e.ok) status = NBEST_BAD_RECORD;
    if ((unsigned)e.row < (unsigned)n) {
      if (sel[(size_t)e.row] != kNoEntry) status = NBEST_BAD_RECORD;
      else sel[(size_t)e.row] = j;
    }
  }
  for (int p = 0; p < n; ++p) {
    int32_t *tk = tok + ((size_t)b * n + p) * T, *tt = ts + ((size_t)b * n + p) * T;
    const int j = sel[(size_t)p];
    bool good = j != kNoEntry && dep[(size_t)j] >= 0;
    int nseg = 0, L = 0;
    if (good) {
      L = dep[(size_t)j];
      int m = L;
      for (int o = j; o >= 0 && m > 0; --o) {
        const int l = lcp[(size_t)o];
        if (l < m) {
          if (!segment_ok(dep[(size_t)o], m)) { good = false; break; }
          seg[(size_t)nseg++] = (uint16_t)o;
          m = l;
        }
      }
    }
    if (j != kNoEntry && !good) status = NBEST_BAD_RECORD;
    if (row_ok) row_ok[p] = good;
    if (!good) L = 0;
    int s = 0;
    for (int q = 0; q < T; ++q) {
      int32_t c = 0, sv = 0;
      if (q < L) {
        s = q == 0 ? seg_find(seg.data(), lcp.data(), nseg, q) : seg_next(seg.data(), lcp.data(), s, q);
        const int o = seg[(size_t)s];
        const uint32_t v = rag[label_index(off[(size_t)o], lcp[(size_t)o], q)];
        c = (int32_t)(v & 0xFFFFu);
        sv = (int32_t)(v >> 16);
      }
      tk[q] = c;
      tt[q] = sv;
    }
  }
  return status;
}

// ---- what nbest.hip exports to the library's host file, and what that file lends it (ctcdecode_amd.hip) -----------------------------
struct NbestDecoderInfo {
  int device;
  int max_lds;
};

}  // namespace ctcnbest

struct ctcd_decoder;
namespace ctcnbest {
int nbest_decoder_info(const ctcd_decoder *d, NbestDecoderInfo *out);  // ctcdecode_amd.hip: the decoder's device and its LDS limit
int nbest_fail(int code, const char *msg);                             // ctcdecode_amd.hip: sets ctcd_last_error, returns code
// nbest.hip: the expansion queued on `stream` (arguments checked by the caller; the caller's device is current).  status: B words that
// are RAISED for malformed items and otherwise left alone, or NULL.  Returns a CTCD_* code.
int launch_nbest_expand(const NbestDecoderInfo &inf, const int32_t *c_hdr, const int32_t *c_ent, const uint32_t *c_labels, unsigned long long n_labels,
                        const float *sc_in, const int32_t *len_in, int B, int beam, int T, int n, int32_t *tok, int32_t *ts, float *sc, int32_t *len,
                        int32_t *status, void *stream);
// whether launch_nbest_expand takes this shape (beam <= kNbestMaxK and the tables fit one workgroup's LDS)
bool nbest_expand_fits(const NbestDecoderInfo &inf, int beam, int n);
}  // namespace ctcnbest
