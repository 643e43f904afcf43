// Host twin of the n-best expansion (ctcdecode_amd/csrc/nbest.h): the product's host expansion of the rows below n, the kernel's
// method run sequentially, and the full host expansion they are compared with, behind a C ABI.  Test infrastructure only.
#include "../../ctcdecode_amd/csrc/nbest.h"

// method 0: expand_item_nbest_host (one row buffer in trie order); 1: rows_by_segments_host (the kernel's segment walk).
// tok / ts: [B, n, T]; row_ok: [B, n] bytes; status: [B] words (0, or NBEST_BAD_RECORD).  Returns the number of malformed items, -1 for
// bad arguments.
extern "C" int ctcnbest_host_expand(const int32_t *hdr, const int32_t *ent, const uint32_t *labels, long long n_labels, int B, int K, int T, int n, int method,
                                    int32_t *tok, int32_t *ts, unsigned char *row_ok, int32_t *status) {
  if (!hdr || !ent || !labels || !tok || !ts || !row_ok || !status || B <= 0 || K <= 0 || T <= 0 || n < 1 || n > K || n_labels < 0) return -1;
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    status[b] = method == 0
                    ? ctcnbest::expand_item_nbest_host(hdr, ent, labels, (unsigned long long)n_labels, b, K, T, n, tok, ts, row_ok + (size_t)b * n)
                    : ctcnbest::rows_by_segments_host(hdr, ent, labels, (unsigned long long)n_labels, b, K, T, n, tok, ts, row_ok + (size_t)b * n);
    bad += status[b] != 0;
  }
  return bad;
}

// the full host expansion of well-formed records (compact_results.h expand_item_host, R == K): tok / ts [B, K, T]
extern "C" int ctcnbest_host_expand_full(const int32_t *hdr, const int32_t *ent, const uint32_t *labels, int B, int K, int T, int32_t *tok, int32_t *ts) {
  if (!hdr || !ent || !labels || !tok || !ts || B <= 0 || K <= 0 || T <= 0) return -1;
  for (int b = 0; b < B; ++b) ctcbeam::expand_item_host(hdr, ent, labels, b, K, T, tok, ts);
  return 0;
}

extern "C" int ctcnbest_host_threads(int n) { return ctcnbest::nbest_threads(n); }
extern "C" long long ctcnbest_host_lds_bytes(int K, int n) { return (long long)ctcnbest::nbest_lds_bytes(K, n, ctcnbest::nbest_threads(n)); }
extern "C" int ctcnbest_host_vec16(int T, unsigned long long tok, unsigned long long ts) { return ctcnbest::nbest_vec16(T, (uintptr_t)tok, (uintptr_t)ts) ? 1 : 0; }
