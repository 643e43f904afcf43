// Host twin of the edit operations (ctcdecode_amd/csrc/editops.h): the routines the kernels of editops.hip compile -- the packed cell
// with and without its direction, a lane's start and step over keys, the slot layout, the counts and the walk's step -- run with 64
// simulated lanes, one after the other, behind a C ABI.  The directions go through a host buffer of exactly the slot's size, allocated
// once per call and reused by every pair, as a wave reuses its slot.  Test infrastructure only.
#include <cstdlib>
#include <cstring>

#include "../../ctcdecode_amd/csrc/editops.h"

namespace {
// the checks of ctcd_edit_counts / ctcd_edit_align.  -> 0, -1 (bad arguments), -2 (beyond a limit)
int ops_check_host(int B, int R, int L, int Q, int Lq) {
  if (B < 0 || R < 0 || L < 0 || Q < 0 || Lq < 0) return -1;
  if ((L < Lq ? L : Lq) > ctcedit::kEditMaxStrip) return -2;
  if ((L < Lq ? Lq : L) > ctcedit::kOpsMaxDim) return -2;
  return 0;
}
}  // namespace

// The whole contract of ctcd_edit_counts on host arrays (y == NULL: pairwise mode).  *pairs: the keys computed.
extern "C" int ctcedit_host_counts(const int32_t *x, const int32_t *x_lens, int B, int R, int L, const int32_t *y, const int32_t *y_lens, int Q, int Lq,
                                   int32_t *out, int32_t *status, long long *pairs) {
  using namespace ctcedit;
  const bool pairwise = y == nullptr;
  if (pairwise) Q = R, Lq = L;
  if (!pairs) return -1;
  *pairs = 0;
  if (B < 0 || R < 0 || L < 0 || Q < 0 || Lq < 0) return -1;
  if (B == 0 || R == 0 || Q == 0) return 0;
  if (!x_lens || !out || (!x && L > 0) || (!pairwise && !y_lens)) return -1;
  if (const int rc = ops_check_host(B, R, L, Q, Lq)) return rc;
  const long long work = pairs_per_item(R, Q, pairwise) * B;
  *pairs = work;
  for (long long w = 0; w < work; ++w) {
    const Pair p = pair_of(w, R, Q, pairwise);
    int32_t cnt[4] = {0, 0, 0, 0};
    if (item_ok_host(x_lens, p.b, R, L, pairwise ? nullptr : y_lens, Q, Lq)) {
      const size_t xi = (size_t)p.b * R + p.i, yj = pairwise ? (size_t)p.b * R + p.j : (size_t)p.b * Q + p.j;
      const int lx = x_lens[xi], ly = pairwise ? x_lens[yj] : y_lens[yj];
      const int key = ops_pair_host(x + xi * (size_t)L, lx, pairwise ? x + yj * (size_t)L : y + yj * (size_t)Lq, ly, false, nullptr, nullptr, 0, nullptr, 0);
      counts_of(key, lx, ly, cnt);
    } else if (status) {
      status[p.b] = EDIT_BAD_ROW;
    }
    int32_t *o = out + (((size_t)p.b * R + p.i) * Q + p.j) * 4;
    o[0] = cnt[0], o[1] = cnt[1], o[2] = cnt[2], o[3] = cnt[3];
    if (pairwise) {
      int32_t *t = out + (((size_t)p.b * R + p.j) * Q + p.i) * 4;
      t[0] = cnt[0], t[1] = cnt[1], t[2] = cnt[3], t[3] = cnt[2];
    }
  }
  if (pairwise)
    for (int b = 0; b < B; ++b) {
      const bool good = item_ok_host(x_lens, b, R, L, nullptr, Q, Lq);
      if (!good && status) status[b] = EDIT_BAD_ROW;
      for (int i = 0; i < R; ++i) {
        int32_t *o = out + (((size_t)b * R + i) * R + i) * 4;
        o[0] = good ? x_lens[(size_t)b * R + i] : 0;
        o[1] = o[2] = o[3] = 0;
      }
    }
  return 0;
}

// The whole contract of ctcd_edit_align on host arrays.  budget: ctcd_set_edit_scratch's (0: the default); *slot_bytes: the size of the
// one slot every pair of the call went through.  fill: the byte the slot holds before the first pair (what a previous call left there
// is nobody's business).
extern "C" int ctcedit_host_align(const int32_t *x, const int32_t *x_lens, int B, int R, int L, const int32_t *y, const int32_t *y_lens, int Q, int Lq,
                                  int32_t *x_to_y, int32_t *y_to_x, int32_t *counts, int32_t *status, long long budget, int fill, long long *slot_bytes) {
  using namespace ctcedit;
  if (!y || !slot_bytes) return -1;
  *slot_bytes = 0;
  if (B < 0 || R < 0 || L < 0 || Q < 0 || Lq < 0 || budget < 0) return -1;
  if (B == 0 || R == 0 || Q == 0) return 0;
  if (!x_lens || !y_lens || (!x && L > 0) || (!x_to_y && L > 0) || (!y_to_x && Lq > 0)) return -1;
  if (const int rc = ops_check_host(B, R, L, Q, Lq)) return rc;
  const size_t sb = ops_slot_bytes(L, Lq);
  *slot_bytes = (long long)sb;
  if (sb && (budget > 0 ? budget : kOpsDefaultScratch) / (long long)sb < 1) return -2;
  void *slot = sb ? std::malloc(sb) : nullptr;  // exactly the slot: a word stored or read outside it is a sanitizer report
  if (sb && !slot) return -3;
  if (sb) std::memset(slot, fill, sb);
  const long long work = pairs_per_item(R, Q, false) * B;
  for (long long w = 0; w < work; ++w) {
    const Pair p = pair_of(w, R, Q, false);
    int32_t cnt[4] = {0, 0, 0, 0};
    int32_t *xm = x_to_y + (size_t)w * L, *ym = y_to_x + (size_t)w * Lq;
    if (item_ok_host(x_lens, p.b, R, L, y_lens, Q, Lq)) {
      const size_t xi = (size_t)p.b * R + p.i, yj = (size_t)p.b * Q + p.j;
      const int lx = x_lens[xi], ly = y_lens[yj];
      const int key = ops_pair_host(x + xi * (size_t)L, lx, y + yj * (size_t)Lq, ly, true, slot, xm, L, ym, Lq);
      counts_of(key, lx, ly, cnt);
    } else {
      if (status) status[p.b] = EDIT_BAD_ROW;
      for (int q = 0; q < L; ++q) xm[q] = -1;
      for (int q = 0; q < Lq; ++q) ym[q] = -1;
    }
    if (counts) {
      int32_t *o = counts + (size_t)w * 4;
      o[0] = cnt[0], o[1] = cnt[1], o[2] = cnt[2], o[3] = cnt[3];
    }
  }
  std::free(slot);
  return 0;
}

extern "C" long long ctcedit_host_slot_bytes(int L, int Lq) { return (long long)ctcedit::ops_slot_bytes(L, Lq); }
extern "C" int ctcedit_host_key_cell(int up, int left, int diag, int32_t a, int32_t b) { return ctcedit::key_cell(up, left, diag, a, b); }
// the cell with its direction (0 pair, 1 the streamed token alone, 2 the strip's token alone)
extern "C" int ctcedit_host_key_cell_dir(int up, int left, int diag, int32_t a, int32_t b, int x_strip, int32_t *dir) {
  int d = -1;
  const int v = ctcedit::key_cell_dir(up, left, diag, a, b, x_strip != 0, &d);
  *dir = d;
  return v;
}
// the key of one pair of plain sequences (no maps)
extern "C" int ctcedit_host_key(const int32_t *a, int la, const int32_t *b, int lb) {
  return ctcedit::ops_pair_host(a, la, b, lb, false, nullptr, nullptr, 0, nullptr, 0);
}
extern "C" void ctcedit_host_counts_of(int key, int lx, int ly, int32_t *out) { ctcedit::counts_of(key, lx, ly, out); }
