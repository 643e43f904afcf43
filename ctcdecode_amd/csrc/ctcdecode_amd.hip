// ctcdecode_amd.hip -- the host side of the CTC prefix beam-search decoder: the C ABI (include/ctcdecode_amd.h), the decoder, stream
// and scorer objects, and the marshalling of binding.cpp:35-101.
//
// Grid mapping (replaces the reference's ThreadPool fan-out, ctc_beam_search_decoder.cpp:259-275): one workgroup per
// utterance; the whole T-step recurrence of that utterance runs inside ONE persistent kernel launch with the beam in
// LDS (a kernel boundary costs ~1.5 us on MI355X -- more than a whole time step should).  The per-utterance algorithm
// is beam_core.h, the workgroup execution policy and the kernel template decode_kernel.h (instantiated in decode_kernels.hip);
// the passes over the caller's rows in front of it are prepass.hip's, and every later feature has a unit of its own.  This file
// decides what a call launches and queues it; its own kernels are a few helpers (result expansion, the math self-check, the
// scorer hook's scatter).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <limits>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/ctcdecode_amd.h"
#define CTC_EXACT_MATH_HOST_TABLES
#include "decode_kernel.h"
#include "exact_math_f64.h"
#include "lm_build.h"
#include "lm_callback.h"
#include "compact_results.h"
#include "device_guard.h"
#include "stream_peek.h"
#include "stream_compact.h"
#include "stream_commit.h"
#include "stream_snapshot.h"
#include "blank_skip.h"
#include "stream_blank_skip.h"
#include "nbest.h"
#include "align.h"
#include "loglik.h"
#include "posterior.h"
#include "greedy.h"
#include "editdist.h"
#include "editops.h"
#include "prepass.h"

namespace {

using namespace ctcbeam;
using namespace ctcprepass;

// (execution policy + kernel template: decode_kernel.h; its instantiations are compiled in decode_kernels.hip)
using namespace ctcdk;
#define CTC_X_EXTERN(PROF_, BIG_, LAYOUT_, PRUNED_, NT_, LM_, OCC2_, G_) extern template __global__ void ctcdk::ctc_beam_decode_kernel<PROF_, BIG_, LAYOUT_, PRUNED_, NT_, LM_, OCC2_>(ctcdk::KernelArgs);
} namespace ctcdk { CTC_KERNEL_LIST(CTC_X_EXTERN) } namespace {
#undef CTC_X_EXTERN
// ... and their addresses by template arguments: what decode_common launches for a planned key (launch_plan.h)
struct KernelEntry {
  KernelKey key;
  const void *fn;
};
#define CTC_X_ENTRY(PROF_, BIG_, LAYOUT_, PRUNED_, NT_, LM_, OCC2_, G_) \
  {{PROF_, BIG_, LAYOUT_, PRUNED_, NT_, (int)(LM_), OCC2_}, (const void *)ctc_beam_decode_kernel<PROF_, BIG_, LAYOUT_, PRUNED_, NT_, LM_, OCC2_>},
const KernelEntry kKernels[] = {CTC_KERNEL_LIST(CTC_X_ENTRY)};
#undef CTC_X_ENTRY
const KernelEntry *kernel_entry(const KernelKey &k) {
  for (const KernelEntry &e : kKernels)
    if (e.key == k) return &e;
  return nullptr;
}
// The exact-shape twins of <0, 0, 1, false, 1024, 0, false> (decode_kernel.h CTC_EXACT_SHAPES; compiled in decode_kernel_exact.hip):
// outside the list the planner chooses from -- decode_common substitutes one for the planned kernel when the call has its shape.
#define CTC_X_EXACT_EXTERN(CODE_, K_, V_, BLANK_, LIVE_) extern template __global__ void ctcdk::ctc_beam_decode_kernel<CODE_, 0, 1, false, 1024, 0, false>(ctcdk::KernelArgs);
} namespace ctcdk { CTC_EXACT_SHAPES(CTC_X_EXACT_EXTERN) } namespace {
#undef CTC_X_EXACT_EXTERN
struct ExactEntry {
  int beam, labels, blank;
  const void *fn;
};
#define CTC_X_EXACT_ENTRY(CODE_, K_, V_, BLANK_, LIVE_) {K_, V_, BLANK_, (const void *)ctc_beam_decode_kernel<CODE_, 0, 1, false, 1024, 0, false>},
const ExactEntry kExactKernels[] = {CTC_EXACT_SHAPES(CTC_X_EXACT_ENTRY)};
#undef CTC_X_EXACT_ENTRY
constexpr KernelKey kExactParent{0, 0, 1, 0, 1024, 0, 0};
// The twin for a call whose planned kernel is `key`, or null: the plain north-star build only, one of the listed shapes exactly,
// nothing pruned (dims), no scorer (the key), the whole utterance in this launch (no stream state, no resumed launch: `whole`).
// Rows streamed from the host never get here: their plan is the PROF 4 build.
const ExactEntry *exact_entry(const KernelKey &key, const Dims &dims, int blank, bool whole) {
  if (!(key == kExactParent) || !whole || dims.use_rank_table || dims.lm) return nullptr;
  for (const ExactEntry &e : kExactKernels)
    if (e.beam == dims.K && e.labels == dims.V && e.labels == dims.Vc_max && e.blank == blank) return &e;
  return nullptr;
}

// Compact results (beam_core.h OutRefs::c_*) -> the reference's tensors: tokens / timesteps [B, K, T], zero outside the
// valid prefixes.  HBM-bound (it writes 8 B per label position of the padded pair).  One workgroup per item; every wave
// takes whole rows, its lanes consecutive label positions (coalesced 256-byte stores).  Label q of DFS entry j is held
// by the nearest entry o <= j with lcp[o] <= q; owner[] (the nearest earlier entry that shares LESS with its own
// predecessor) lets the search skip runs of entries, as in the decode kernel's own back-trace.
constexpr int kExpandMaxK = 4096;  // entries whose tables fit LDS; wider beams take the generic slow loop
__global__ void __launch_bounds__(1024) expand_compact_kernel(const int32_t *hdr, const int32_t *ent, const uint32_t *rag, int K, int T,
                                                              int32_t *tok, int32_t *ts) {
  extern __shared__ int esm[];
  int *lcp = esm, *dep = esm + K, *off = esm + 2 * K, *row = esm + 3 * K, *owner = esm + 4 * K;
  unsigned *used = (unsigned *)(esm + 5 * K);  // K bits
  const int b = (int)blockIdx.x;
  const int nres = hdr[(size_t)b * 4];
  int32_t *tk0 = tok + (size_t)b * K * T, *ts0 = ts + (size_t)b * K * T;
  for (int i = (int)threadIdx.x; i < (K + 31) / 32; i += (int)blockDim.x) used[i] = 0u;
  for (int j = (int)threadIdx.x; j < nres; j += (int)blockDim.x) {
    const int4 e = *reinterpret_cast<const int4 *>(ent + ((size_t)b * K + j) * 4);
    row[j] = e.x; lcp[j] = j == 0 ? 0 : e.y; dep[j] = e.z; off[j] = e.w;
  }
  __syncthreads();
  for (int j = (int)threadIdx.x; j < nres; j += (int)blockDim.x) {
    int o = j - 1;
    const int l = lcp[j];
    while (o >= 0 && lcp[o] >= l) --o;
    owner[j] = o < 0 ? 0 : o;
    atomicOr(&used[row[j] >> 5], 1u << (row[j] & 31));
  }
  __syncthreads();
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, nw = (int)blockDim.x >> 6;
  for (int j = wave; j < K; j += nw) {
    if (j < nres) {
      int32_t *tk = tk0 + (size_t)row[j] * T, *tt = ts0 + (size_t)row[j] * T;
      const int dj = dep[j];
      for (int q = lane; q < T; q += 64) {
        int32_t c = 0, sv = 0;
        if (q < dj) {
          int o = j;
          while (lcp[o] > q) o = owner[o];  // (lcp[0] = 0 ends the walk)
          const uint32_t v = rag[(uint32_t)off[o] + (uint32_t)(q - lcp[o])];
          c = (int32_t)(v & 0xFFFFu);
          sv = (int32_t)(v >> 16);
        }
        tk[q] = c;
        tt[q] = sv;
      }
    }
    // rows without a result: row index j doubles as the row to check
    if (!((used[j >> 5] >> (j & 31)) & 1u)) {
      int32_t *tk = tk0 + (size_t)j * T, *tt = ts0 + (size_t)j * T;
      for (int q = lane; q < T; q += 64) { tk[q] = 0; tt[q] = 0; }
    }
  }
}

__global__ void debug_math_kernel(int mode, uint32_t start, uint32_t stride, const float *xs, const float *ys, float *out,
                                  size_t n, const uint64_t *tables) {
  __shared__ uint64_t tbl[64];
  if (threadIdx.x < 64) tbl[threadIdx.x] = tables[threadIdx.x];
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (mode == 2) {
    out[i] = ctcmath::lse(xs[i], ys[i], tbl);
  } else {
    const float x = ctcmath::bits_to_f32(start + (uint32_t)i * stride);
    out[i] = mode == 0 ? ctcmath::expf_nonpos(x, tbl) : ctcmath::logf_normal(x, tbl);
  }
}

// binary64 log / exp / log_sum_exp of exact_math_f64.h on float images (modes 3..6 of ctcd_debug_math_check)
__global__ void debug_math64_kernel(int mode, uint32_t start, uint32_t stride, const float *xs, const float *ys, uint64_t *out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r;
  if (mode == 6) {
    r = ctcmath::lse_f64((double)xs[i], (double)ys[i], ctcmath::tables64());
  } else {
    const double x = (double)ctcmath::bits_to_f32(start + (uint32_t)i * stride);
    r = mode == 3   ? ctcmath::log_f64(x, ctcmath::tables64())
        : mode == 4 ? ctcmath::log_f64(x + (double)FLT_MIN, ctcmath::tables64())
                    : ctcmath::exp_f64(x, ctcmath::tables64());
  }
  out[i] = ctcmath::f64_to_bits(r);
}

// ------------------------------------------------------------------------------------------------ host side
thread_local std::string g_err;
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return fail(CTCD_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
  } while (0)

// Every C ABI entry point works on the decoder's device and puts the caller's current device back on exit (device_guard.h).
using ctcdev::DeviceGuard;
#define CTC_ON_DEVICE(dev)  \
  DeviceGuard guard_(dev);  \
  HIP_TRY(guard_.err)

struct Buf {
  void *p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return CTCD_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail(CTCD_EHIP, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    cap = bytes;
    return CTCD_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

}  // namespace

// A few host threads that stay parked between calls (expanding 2 x [B, K, T] on one thread would take longer than the decode)
struct HostPool {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv, done_cv;
  std::function<void(int)> job;
  int n_items = 0, next = 0, running = 0;
  unsigned long long epoch = 0;
  bool stop = false;
  void start(int n) {  // (also grows a running pool: the new threads start behind the jobs already done)
    unsigned long long e;
    { std::lock_guard<std::mutex> g(mu); e = epoch; }
    for (int i = 0; i < n; ++i) th.emplace_back([this, e] { loop(e); });
  }
  void loop(unsigned long long seen) {
    for (;;) {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return stop || epoch != seen; });
      if (stop) return;
      seen = epoch;
      for (;;) {
        if (next >= n_items) break;
        const int i = next++;
        lk.unlock();
        job(i);
        lk.lock();
      }
      if (--running == 0) done_cv.notify_all();
    }
  }
  void run(int items, std::function<void(int)> f) {
    if (th.empty() || items <= 1) { for (int i = 0; i < items; ++i) f(i); return; }
    std::unique_lock<std::mutex> lk(mu);
    job = std::move(f); n_items = items; next = 0; running = (int)th.size(); ++epoch;
    cv.notify_all();
    done_cv.wait(lk, [&] { return running == 0; });
  }
  ~HostPool() {
    { std::lock_guard<std::mutex> g(mu); stop = true; }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
};

struct ctcd_decoder {
  int device = 0;
  Buf c_hdr, c_ent, c_rag, c_cnt, c_sc, c_ln;  // compact results of the host-tensor entry points
  void *h_stage = nullptr;  // page-locked staging for them
  size_t h_stage_cap = 0;
  HostPool *workers = nullptr;
  int threads = 0;  // 0 = choose per call from the number of candidate slots
  int max_lds = 0;
  int cu_count = 0;
  long long lds_floor = -1;  // CTCD_LDS_FLOOR (experiments): dynamic LDS bytes every decode launch asks for at least
  int exact_shape = -1;      // ctcd_set_exact_shape: -1 = an exact-shape twin wherever a call qualifies, 0 = never, 1 = required
  int last_exact = 0;        // ctcd_last_exact_shape: the last launch ran a twin
  int cu_sharing = -1;       // ctcd_set_cu_sharing: 1 = always launch the two-workgroups-per-CU build, 0 = never, -1 = when B > #CUs
  Buf pool, status, tables, logp, lsm, flags, stage_in, stage_out, pr_cnt, pr_ch, pr_lp, pr_ml, far, st_args;
  Buf prune_in, prune_out, st_lens;  // own staging: the host-pointer entry points keep their tensors in stage_in/out
  Buf cb_blocks, cb_ctl;             // scorer hook: the temporary streams' blocks of a one-shot decode; per-item control words
  int32_t *h_cb = nullptr;           // ... and, page-locked, what a round reports: [status | frames done | #misses]
  size_t h_cb_items = 0;
  long long prune_flagged_rows = 0;  // frames of the last call the fast prune pass flagged (settled by prune_resolve_kernel)
  unsigned *h_flagged = nullptr;     // page-locked: that count, copied behind the kernels
  bool flagged_pending = false;
  bool resolve_in_global = false;    // tests: the std::sort replay's arrays in global memory whatever the row length
  bool tables_ready = false;
  bool timing = false;
  bool profile = false, dbg_on = false;
  bool no_fixed_layout = false;  // debugging: always use the run-time workspace layout
  bool no_prune_reg = false;     // debugging / tests: the two-sweep form of the workgroup prune kernel
  bool no_hook_wait = false;     // tests: a callback scorer's launches end at a miss (the form of rounds 4-5) instead of waiting for the answer
  int last_cb_waits = 0;         // answer batches the last call's launches were handed while they waited
  bool no_lmq_filter = false;    // tests / measurements: a callback scorer's kernels queue every miss (ctcd_set_scorer_filter; LmView::cb = 2)
  long long last_pairs[3] = {0, 0, 0};  // scorer hook, the last decode: queued pairs | windows asked | repeats of the same item (ctcd_last_scorer_pairs)
  bool no_fused_logits = false;  // tests: raw logits always through the one-wave log_softmax pass and the separate prune
  int in_dtype = CTCD_DTYPE_F32;       // ctcd_set_input_dtype: the element type of probs / logits on every entry point
  int last_in_dtype = CTCD_DTYPE_F32;  // the element type the last call's pre-passes read (ctcd_last_input_dtype)
  int launch_order = CTCD_ORDER_BATCH; // ctcd_set_launch_order
  Buf order;                           // length order: [ticket | permutation] of a call's first launch, then of a resumed launch (scorer hook)
  int last_order_items = 0;            // items of the last one-shot call's permutation in `order` (0: that call ran in batch order)
  hipEvent_t ev_order = nullptr;       // recorded behind that call's order pass (ctcd_debug_last_launch_order waits for it)
  Buf prof, dbg, tl;
  int tl_f0 = 0, tl_nf = 0;
  int status_items = 0;          // items of the launch whose status words (and shape statistic) are in d->status
  bool tl_armed = false;
  // phase A1's four-entries-per-wave subtree search (decode_kernel.h kQuarters): -1 = chosen per launch from the beam shape the
  // last checked launch reported (chains: on), 0 / 1 = forced
  int subtree_mode = -1;
  bool subtree_on = false;       // the automatic choice for the next launch
  const KernelEntry *last_kernel = nullptr;  // the kernel the last launch used (null: none yet)
  // the pre-pass kernels the last call queued (ctcd_debug_last_prepass): elementwise | log_softmax | prune | prune_resolve (null: none)
  const void *pre_fn[4] = {nullptr, nullptr, nullptr, nullptr};
  bool pre_resolve_global = false;  // ... and the route of that prune_resolve_kernel: its arrays in global memory (else LDS)
  int last_cb_rounds = 0;        // scorer hook: launches the last decode through a callback scorer took (ctcd_last_scorer_rounds)
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;  // decode kernel | vocabulary-prune pass
  bool prune_timed = false;
  // streamed input of the host-tensor entry point: rows cross PCIe frame block by frame block while the kernel runs
  void *fg_in = nullptr;          // fine-grained (uncached) device memory: [frames-arrived counter | rows | seq_lens]
  size_t fg_in_cap = 0;
  int *h_cnt = nullptr;           // page-locked: the counter values the copy stream writes behind each block
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_in = nullptr;
  bool no_input_streaming = false;
  bool stall_input_test = false;
  bool general_lm_kernel = false;  // CTCD_GENERAL_LM_KERNEL=1: word models, too, run the scorer instantiations that serve every model
  bool input_timed_out = false;   // set by ctcd_check_status when an utterance reports ST_INPUT_TIMEOUT
  long long mirror_cap_override = -1;  // tests: labels the host mirror of the compact results holds (-1: a third of the worst case)
  hipStream_t last_stream = nullptr;  // the stream of the last decode launch (ctcd_check_status reads the status words on it)
  // streaming calls: their per-item arguments (block pointers, pool capacities, end-of-stream flags, chunk lengths) travel
  // in ONE copy from page-locked staging -- two slots, an event each: a chunk call costs no stream synchronisation
  char *h_stargs[2] = {nullptr, nullptr};
  size_t h_stargs_cap = 0;
  hipEvent_t ev_stargs[2] = {nullptr, nullptr};
  unsigned long long stream_calls = 0;
  // ctcd_stream_peek: its per-item arguments [block pointers | pool capacities | since] travel like a chunk call's (two page-locked
  // slots, an event each); its status words are its own, so that a peek between unchecked chunks does not hide their outcome
  Buf peek_args, peek_status;
  char *h_pkargs[2] = {nullptr, nullptr};
  size_t h_pkargs_cap = 0;
  hipEvent_t ev_pkargs[2] = {nullptr, nullptr};
  unsigned long long peek_calls = 0;
  int peek_items = 0;                 // items of a queued peek whose status words nobody has looked at yet (0: none)
  hipStream_t peek_stream = nullptr;  // ... and the stream it was queued on
  // ctcd_stream_compact: the new layouts are gathered here before they go back into the streams' blocks; its per-item arguments
  // and what its kernels report live in one page-locked region both sides read and write in place (the call is synchronous)
  Buf cp_scratch;
  char *h_cp = nullptr;
  size_t h_cp_cap = 0;
  long long compact_min_nodes = 0;    // ctcd_set_stream_compaction: 0 = a stream that outgrows its pool doubles it, as ever
  // ctcd_set_stream_blank_skip (stream_blank_skip.h): the filter in front of every chunk of this decoder's streams.  sk_rows / sk_kept /
  // sk_lsm: the chunk's kept rows, their chunk-local indices and -- raw logits -- the float32 log-softmax rows the scan reads.  h_sk: one
  // page-locked region both sides read and write in place, [scan table | chunk lengths | kept counts] (a filtered chunk call waits for
  // the counts before it launches its decode, so the region is free when the call returns) and, behind them, the remap table of the
  // last call that reported time steps: ev_sk_tab is recorded behind that call's remap kernel and waited for before the table changes.
  bool sk_on = false;
  float sk_cmp_prob = 0.f, sk_cmp_log = 0.f;
  Buf sk_rows, sk_kept, sk_lsm;
  char *h_sk = nullptr;
  size_t h_sk_items = 0;
  hipEvent_t ev_sk_tab = nullptr, ev_sk[4] = {nullptr, nullptr, nullptr, nullptr};  // ev_sk: filter start | end, remap start | end (ctcd_set_timing)
  bool sk_tab_busy = false, sk_timed = false, sk_remap_timed = false;
  float sk_wait_ms = 0.f;
  long long sk_last[2] = {0, 0};      // frames considered | kept by the last filtered chunk call (ctcd_last_stream_blank_skip)
  std::mutex mu_skip;                 // a filtered streaming call holds it from its scan to its remap
  // ctcd_ctc_align (align.h): the back-pointer slots of its persistent workgroups, the float32 log-softmax rows of raw logits, the
  // budget of the former (ctcd_set_align_scratch; 0 = the default) and the grid of the last call (ctcd_last_align_grid)
  Buf al_bp, al_lsm;
  long long al_budget = 0, al_grid = 0;
  // ctcd_ctc_loglik (loglik.h): the cap of its grid (ctcd_set_loglik_grid; 0 = the default) and the widest grid of the last call
  long long ll_cap = 0, ll_grid = 0;
  // ctcd_ctc_posteriors (posterior.h): the slots that keep the forward values between its two walks, their budget
  // (ctcd_set_posterior_scratch; 0 = the default) and the grid of the last call (ctcd_last_posterior_grid)
  Buf po_alpha;
  long long po_budget = 0, po_grid = 0;
  // ctcd_greedy_decode (greedy.h): the frame records its argmax pass leaves its collapse pass
  Buf gr_frames;
  // ctcd_edit_distance (editdist.h): the pairs its last call ran (ctcd_last_edit_pairs)
  long long ed_pairs = 0;
  // ... the cap of its grid (ctcd_set_edit_grid; 0 = the default) and the workgroups of its last launch (ctcd_last_edit_grid)
  long long ed_cap = 0, ed_grid = 0;
  // ctcd_edit_align (editops.h): the back-pointer slots of its waves, their budget (ctcd_set_edit_scratch; 0 = the default) and the
  // slots of the last call (ctcd_last_edit_slots)
  Buf ed_bp;
  long long ed_budget = 0, ed_slots = 0;
  // ctcd_greedy_stream_decode (greedy.h "live streams"): a chunk call's per-stream arguments travel like ctcd_stream_decode's (two
  // page-locked slots, an event each, one copy per call)
  Buf gs_args;
  char *h_gsargs[2] = {nullptr, nullptr};
  size_t h_gsargs_cap = 0;
  hipEvent_t ev_gsargs[2] = {nullptr, nullptr};
  unsigned long long gs_calls = 0;
  std::mutex mu;
  std::mutex mu_host;  // the host-tensor entry points: compact buffers, page-locked staging and the worker threads are per decoder
};

// what the blank-frame filter's entry points (blank_skip.hip) need of this file: the decoder's device and input dtype, ctcd_last_error
namespace ctcskip {
int skip_decoder_info(const ctcd_decoder *d, SkipDecoderInfo *out) {
  if (!d || !out) return fail(CTCD_EINVAL, "decoder == NULL");
  out->device = d->device;
  out->in_dtype = d->in_dtype;
  return CTCD_OK;
}
int skip_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }
}  // namespace ctcskip

// ... and the n-best expansion's (nbest.hip): the decoder's device and LDS limit
namespace ctcnbest {
int nbest_decoder_info(const ctcd_decoder *d, NbestDecoderInfo *out) {
  if (!d || !out) return fail(CTCD_EINVAL, "decoder == NULL");
  out->device = d->device;
  out->max_lds = d->max_lds;
  return CTCD_OK;
}
int nbest_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }
}  // namespace ctcnbest

// ... and the forced alignment's (align.hip): device, input dtype and scratch budget; its two decoder-owned buffers
namespace ctcalign {
int align_decoder_info(const ctcd_decoder *d, AlignDecoderInfo *out) {
  if (!d || !out) return fail(CTCD_EINVAL, "decoder == NULL");
  out->device = d->device;
  out->in_dtype = d->in_dtype;
  out->budget = d->al_budget;
  return CTCD_OK;
}
int align_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }
int align_scratch(ctcd_decoder *d, size_t bytes, void **p) {
  std::lock_guard<std::mutex> lock(d->mu);
  if (const int rc = d->al_bp.ensure(bytes)) return rc;
  *p = d->al_bp.p;
  return CTCD_OK;
}
int align_lsm_rows(ctcd_decoder *d, const void *logits, const int32_t *seq_lens, int B, int T, int V, void *stream, const float **rows) {
  {
    std::lock_guard<std::mutex> lock(d->mu);
    if (const int rc = d->al_lsm.ensure((size_t)B * T * V * sizeof(float))) return rc;
  }
  *rows = (const float *)d->al_lsm.p;
  return ctcd_log_softmax(d, (const float *)logits, seq_lens, B, T, V, (float *)d->al_lsm.p, stream);
}
void align_note_grid(ctcd_decoder *d, long long grid) { d->al_grid = grid; }
}  // namespace ctcalign

// ... and the log-likelihood's (loglik.hip), beyond the alignment's hooks: the cap of its grid and the device's compute units
namespace ctcloglik {
int loglik_decoder_info(const ctcd_decoder *d, LoglikDecoderInfo *out) {
  if (!d || !out) return fail(CTCD_EINVAL, "decoder == NULL");
  out->cap = d->ll_cap;
  out->cus = d->cu_count;
  return CTCD_OK;
}
void loglik_note_grid(ctcd_decoder *d, long long grid) { d->ll_grid = grid; }
}  // namespace ctcloglik

// ... and the label posteriors' (posterior.hip): the budget of their scratch, and the scratch
namespace ctcpost {
long long post_budget(const ctcd_decoder *d) { return d->po_budget; }
int post_scratch(ctcd_decoder *d, size_t bytes, void **p) {
  std::lock_guard<std::mutex> lock(d->mu);
  if (const int rc = d->po_alpha.ensure(bytes)) return rc;
  *p = d->po_alpha.p;
  return CTCD_OK;
}
void post_note_grid(ctcd_decoder *d, long long grid) { d->po_grid = grid; }
}  // namespace ctcpost

// ... and the edit distance's (editdist.hip): the decoder's device and compute units, and the count of its last call's pairs
namespace ctcedit {
int edit_decoder_info(const ctcd_decoder *d, EditDecoderInfo *out) {
  if (!d || !out) return fail(CTCD_EINVAL, "decoder == NULL");
  out->device = d->device;
  out->cus = d->cu_count;
  out->cap = d->ed_cap;
  return CTCD_OK;
}
int edit_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }
void edit_note_pairs(ctcd_decoder *d, long long pairs, long long grid) {
  d->ed_pairs = pairs;
  d->ed_grid = grid;
}
// ... and the edit operations' (editops.hip): the budget of the back-pointer scratch, the scratch, and the slots of the last call
long long edit_budget(const ctcd_decoder *d) { return d->ed_budget; }
int edit_scratch(ctcd_decoder *d, size_t bytes, void **p) {
  std::lock_guard<std::mutex> lock(d->mu);
  if (const int rc = d->ed_bp.ensure(bytes)) return rc;
  *p = d->ed_bp.p;
  return CTCD_OK;
}
void edit_note_slots(ctcd_decoder *d, long long slots) { d->ed_slots = slots; }
}  // namespace ctcedit

// ... and the greedy decode's (greedy.hip), beyond the alignment's hooks: its frame records
namespace ctcgreedy {
int greedy_scratch(ctcd_decoder *d, size_t bytes, void **p) {
  std::lock_guard<std::mutex> lock(d->mu);
  if (const int rc = d->gr_frames.ensure(bytes)) return rc;
  *p = d->gr_frames.p;
  return CTCD_OK;
}
// ... and its streams' (greedy_stream.hip): a chunk call's per-stream arguments, staged in page-locked memory and sent with ONE
// asynchronous copy, as ctcd_stream_decode sends its own
int greedy_stream_upload(ctcd_decoder *d, const void *src, size_t bytes, void *stream, void **dev) {
  std::lock_guard<std::mutex> lock(d->mu);
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (const int rc = d->gs_args.ensure(2 * need)) return rc;
  if (d->h_gsargs_cap < need) {
    for (int i = 0; i < 2; ++i) {
      if (d->ev_gsargs[i]) HIP_TRY(hipEventSynchronize(d->ev_gsargs[i]));
      if (d->h_gsargs[i]) (void)hipHostFree(d->h_gsargs[i]);
      d->h_gsargs[i] = nullptr;
      d->h_gsargs_cap = 0;
      HIP_TRY(hipHostMalloc((void **)&d->h_gsargs[i], need, hipHostMallocDefault));
      if (!d->ev_gsargs[i]) HIP_TRY(hipEventCreateWithFlags(&d->ev_gsargs[i], hipEventDisableTiming));
    }
    d->h_gsargs_cap = need;
  }
  const int slot = (int)(d->gs_calls++ & 1);
  HIP_TRY(hipEventSynchronize(d->ev_gsargs[slot]));  // (the copy of two calls ago: long done)
  memcpy(d->h_gsargs[slot], src, bytes);
  // (the slots' offsets follow the capacity of the page-locked end, which only grows with the device end)
  char *db = (char *)d->gs_args.p + (size_t)slot * d->h_gsargs_cap;
  HIP_TRY(hipMemcpyAsync(db, d->h_gsargs[slot], bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipEventRecord(d->ev_gsargs[slot], (hipStream_t)stream));
  *dev = db;
  return CTCD_OK;
}
}  // namespace ctcgreedy

// One audio stream's parked decoder state (ctcd_stream_*): a single HBM block [header | beam arrays | node pool].
struct ctcd_stream {
  unsigned long long seen_in_call = 0;  // ctcd_stream_decode: "this state is already part of the current call" in O(1)
  int device = 0;
  ctcd_scorer *scorer = nullptr;  // DecoderState is created with its scorer (binding.cpp:243-261)
  char *block = nullptr;
  size_t bytes = 0;
  int V = 0, beam = 0;
  long long frames = 0;      // frames fed so far (host mirror of the header word)
  long long cap_frames = 0;  // the node pool holds cap_frames * beam + 1 nodes
  // ctcd_stream_compact (stream_compact.h): the nodes the last compaction left and the frame it ran at -- the pool count is at most
  // base_nodes + (frames - base_frames) * beam; (1, 0) until the first one: frames * beam + 1
  long long base_nodes = 1, base_frames = 0;
  long long hint_frames = 0;  // the capacity the stream was created with: a compacted stream does not shrink below it
  long long committed = 0;    // ctcd_stream_commit (stream_commit.h): labels handed out so far -- everything the stream reports counts from there
  // the blank-frame filter of live streams (stream_blank_skip.h): `frames` counts the frames decoded, the kept ones; `seen` the frames
  // fed.  map[i] = index among the seen frames of the i-th kept one, i < frames: an allocation of its own (compaction and doubling move
  // the block), grown by doubling, never shrunk, freed with the stream.  filtered: the stream took its first chunk through the filter.
  bool filtered = false;
  long long seen = 0;
  int32_t *map = nullptr;
  long long map_cap = 0;
};

// The external scorer (ctcdecode/src/scorer.h:41-110, created by paddle_get_scorer, binding.cpp:143-150): built on the host
// from the ARPA file (lm_build.h), its tables mirrored into the HBM of one device (lm_tables.h).
// Helper threads of a callback scorer whose callback may be called from several threads at once (ctcd_scorer_set_callback_threads): while a
// waiting launch is being served they spin on a generation counter, take every P-th window of the batch the serving thread publishes and
// report once per batch; between launches they sleep.  The serving thread takes its own share, so P threads ask P windows at a time.
struct CbAskPool {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv;
  bool active = false, stop = false;           // (under mu)
  std::atomic<unsigned long long> gen{0};      // batches published
  std::atomic<int> acks{0};                    // helpers done with the current batch
  ctclm::CallbackLm *cl = nullptr;
  ctclm::CallbackLm::Ask *batch = nullptr;
  int n = 0;
  int parts() const { return (int)th.size() + 1; }
  void worker(int w) {
    unsigned long long seen = gen.load(std::memory_order_acquire);
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return active || stop; });
        if (stop) return;
      }
      for (unsigned spin = 0;; ++spin) {
        const unsigned long long g = gen.load(std::memory_order_acquire);
        if (g != seen) {
          seen = g;
          const int P = parts();
          for (int i = w; i < n; i += P) cl->ask(batch[i]);
          acks.fetch_add(1, std::memory_order_release);
          spin = 0;
        } else if ((spin & 4095) == 4095) {
          std::lock_guard<std::mutex> lk(mu);
          if (!active || stop) break;
        }
        __builtin_ia32_pause();
      }
    }
  }
  void start(int threads, ctclm::CallbackLm *c) {
    shutdown();
    cl = c;
    stop = false;
    for (int w = 1; w < threads; ++w) th.emplace_back([this, w] { worker(w); });
  }
  void shutdown() {
    { std::lock_guard<std::mutex> lk(mu); stop = true; active = false; }
    cv.notify_all();
    for (auto &t : th) t.join();
    th.clear();
  }
  void begin() { if (th.empty()) return; { std::lock_guard<std::mutex> lk(mu); active = true; } cv.notify_all(); }
  void end() { if (th.empty()) return; std::lock_guard<std::mutex> lk(mu); active = false; }
  // asks batch[0 .. n): this thread's share here, the helpers' shares beside it (all of them in this thread when the batch is short)
  void ask_all(ctclm::CallbackLm::Ask *b, int count) {
    if (th.empty() || count < 4) { for (int i = 0; i < count; ++i) cl->ask(b[i]); return; }
    batch = b; n = count;
    acks.store(0, std::memory_order_relaxed);
    gen.fetch_add(1, std::memory_order_release);
    const int P = parts();
    for (int i = 0; i < count; i += P) cl->ask(b[i]);
    while (acks.load(std::memory_order_acquire) != P - 1) __builtin_ia32_pause();
  }
};

struct ctcd_scorer {
  ctclm::HostScorer host;
  int device = 0;
  char *blob = nullptr;      // one HBM allocation holding every table
  unsigned long long fingerprint = 0;  // of the tables as uploaded (stream_snapshot.h scorer_fingerprint): images of its streams carry it
  ctclm::LmView dview;       // the tables as the kernel sees them (alpha / beta are refreshed at every launch)
  // Host-side scorer hook (ctcd_scorer_create_callback, lm_callback.h): the device tables are a cache of the callback's
  // answers -- grown between launches (cb_sync); `host` keeps the scalar facts the accessors report
  ctclm::CallbackLm *cbl = nullptr;
  char *cb_ng = nullptr, *cb_st = nullptr, *cb_uni = nullptr, *cb_miss = nullptr;  // cache slots | zeroed state arrays | NaN unigrams | miss list + counter
  size_t cb_ng_slots = 0, cb_st_cap = 0;
  char *cb_stage = nullptr;  // dirty cache slots of a round, sent with ONE copy and scattered by a kernel: [indices | slots]
  size_t cb_stage_cap = 0;   // ... slots it holds
  char *cb_stage_hp = nullptr;  // ... its page-locked host end
  hipEvent_t cb_stage_ev = nullptr;  // ... and the last copy out of it
  std::mutex cb_mu;          // one decode at a time mutates the cache
  // page-locked, device-visible block of the launches that wait for their answers (cb_rounds): [log length | workgroup reports |
  // pairs answered per item | miss list | log: slot indices | log: slots]
  char *h_live = nullptr, *d_live = nullptr;  // host address / the same memory as the device addresses it
  unsigned live_miss_hw = 0;                  // miss-list entries the last launch may have written (reset to the sentinel before the next)
  std::vector<uint32_t> live_stamp;           // per cache slot: the waiting launch whose log holds it
  std::vector<unsigned long long> live_memo;  // (state, word) pairs recently put into / found in that log (direct-mapped, 512 KB)
  std::vector<uint32_t> live_memo_at;         // ... and their slots
  std::vector<uint64_t> pair_seen;            // per cache slot: (decode << 32 | the item that queued it first in that decode): ctcd_last_scorer_pairs
  uint32_t pair_call = 0;
  uint32_t live_launch = 0;
  CbAskPool ask_pool;                         // helper threads of a thread-safe callback (none unless asked for)
};
constexpr uint32_t kCbMissCap = 1u << 18;  // queued (state, word) pairs per round (2 MB); more are dropped and asked again
constexpr uint32_t kCbLogCap = 1u << 21;   // cache slots one waiting launch can be handed (40 MB of page-locked memory)
constexpr size_t kCbLiveSlots0 = (size_t)1 << 22;   // a waiting launch cannot have its tables moved: they start with room for 2 M windows (64 MB of HBM) ...
constexpr size_t kCbLiveStates0 = (size_t)1 << 22;  // ... and 4 M states (two zeroed arrays, 32 MB)
constexpr uint32_t kCbLiveItems = 1u << 16;
constexpr size_t kLiveOffDone = 256, kLiveOffAns = kLiveOffDone + (size_t)kCbLiveItems * 4, kLiveOffMiss = kLiveOffAns + (size_t)kCbLiveItems * 4,
                 kLiveOffIdx = kLiveOffMiss + (size_t)kCbMissCap * sizeof(ctclm::MissEntry), kLiveOffSlot = kLiveOffIdx + (size_t)kCbLogCap * 4,
                 kLiveBytes = kLiveOffSlot + (size_t)kCbLogCap * sizeof(ctclm::NgSlot);

namespace {

struct CompactOut {          // compact result delivery (beam_core.h OutRefs::c_*); all device pointers
  int32_t *hdr, *ent;
  uint32_t *rag;
  unsigned *count;
  unsigned cap;
  // mirrors in page-locked host memory the kernel writes a finished utterance's results to (OutRefs::m_*); null: none
  int32_t *m_hdr = nullptr, *m_ent = nullptr, *m_done = nullptr;
  uint32_t *m_rag = nullptr;
  unsigned m_cap = 0;
};

struct StreamCall {          // extra arguments of a streaming decode (lens: the chunk lengths, host memory)
  ctcd_stream **states;
  const unsigned char *is_eos;  // host
  int out_T;
  const int32_t *lens;          // host: frames of this chunk per item
  bool any_eos;
  // resumed launches of the scorer hook (decode_lm_callback): the results of items that finished in an earlier launch stay
  // (nothing is zero-filled), every item starts at its own frame of the rows, and reports how far its parked state got
  bool no_clear = false;
  const int *frame_off = nullptr;   // device, [B]
  int *frames_done = nullptr;       // device, [B]
  const int32_t *row_lens = nullptr;  // device, [B]: frame_off + lens = the rows the pre-passes (log conversion, pruning) cover
  const char *live = nullptr;         // the scorer's page-locked block as the device sees it (ctcd_scorer::d_live): the launch waits for its answers
  bool one_shot = false;              // the launches of a one-shot decode through a callback scorer: they follow ctcd_set_launch_order
  int in_dtype = -1;                  // >= 0: the element type of `probs` for this call, whatever ctcd_set_input_dtype says (a filtered chunk's rows)
};

std::atomic<unsigned long long> g_stream_call_id{0};
// (the parked arrays are always laid out for the LM tier's larger set: a stream block is sized once, before its scorer matters)
size_t stream_pool_offset(int beam) { return ((size_t)(SH_WORDS + kStateArraysLm * (size_t)beam) * 4 + 255) / 256 * 256; }
// a stream block holds [header | beam arrays | node pool (nodes * 12 B) | express pointers (nodes * 4 B) | high parts of the
// nodes' time steps (nodes * 4 B, zero until the stream passes frame 65535)]
size_t stream_nodes(long long frames, int beam) { return (size_t)frames * beam + 1; }
size_t stream_block_bytes(long long cap_frames, int beam) {
  return stream_pool_offset(beam) + stream_nodes(cap_frames, beam) * (sizeof(PoolNode) + 2 * sizeof(int));
}
size_t stream_thi_offset(long long cap_frames, int beam) {
  return stream_pool_offset(beam) + stream_nodes(cap_frames, beam) * (sizeof(PoolNode) + sizeof(int));
}

int check_args(int B, int T, int V, int beam, int cutoff_top_n, int blank_id, const void *probs, const void *tok,
               const void *ts, const void *sc, const void *ln) {
  if (B < 0 || T < 0 || V <= 0 || beam <= 0 || cutoff_top_n <= 0) return fail(CTCD_EINVAL, "B, T >= 0 and V, beam_width, cutoff_top_n > 0 required");
  if (blank_id < 0 || blank_id >= V) return fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (beam > kMaxBeam) return fail(CTCD_EUNSUPPORTED, "beam_width > 16383");
  if (V > kMaxVocab) return fail(CTCD_EUNSUPPORTED, "vocabulary > 65534");
  if ((long long)beam * T + 1 > 0x7fffffffLL) return fail(CTCD_EUNSUPPORTED, "beam_width * T too large");
  if (B > 0 && T > 0 && (!probs || !tok || !ts)) return fail(CTCD_EINVAL, "null tensor");
  if (B > 0 && (!sc || !ln)) return fail(CTCD_EINVAL, "null tensor");
  return CTCD_OK;
}

}  // namespace

extern "C" {

const char *ctcd_last_error(void) { return g_err.c_str(); }
const char *ctcd_version(void) { return "ctcdecode_amd 0.1 (gfx950)"; }

int ctcd_workgroup_lds_bytes(int beam, int V, int cutoff_top_n, double cutoff_prob) {
  if (beam <= 0 || V <= 0 || cutoff_top_n <= 0) return CTCD_EINVAL;
  Work w;
  const size_t n = carve<0>(w, nullptr, nullptr, make_dims(beam, V, cutoff_top_n, used_cutoff_prob(cutoff_prob)), nullptr);
  return n > 0x7fffffffu ? 0x7fffffff : (int)n;
}

int ctcd_create(ctcd_decoder **out, int device_id) {
  if (!out) return fail(CTCD_EINVAL, "out == NULL");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail(CTCD_EINVAL, "no such HIP device");
  ctcd_decoder *d = new ctcd_decoder;
  d->device = device_id;
  int v = 0;
  HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id));
  d->max_lds = v;
  HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device_id));
  d->cu_count = v;
  if (const char *e = getenv("CTCD_LDS_FLOOR")) d->lds_floor = atoll(e);
  if (const char *e = getenv("CTCD_NO_INPUT_STREAMING")) d->no_input_streaming = atoi(e) != 0;
  if (const char *e = getenv("CTCD_GENERAL_LM_KERNEL")) d->general_lm_kernel = atoi(e) != 0;
  *out = d;
  return CTCD_OK;
}

void ctcd_destroy(ctcd_decoder *d) {
  if (!d) return;
  DeviceGuard guard_(d->device);
  if (d->fg_in) (void)hipFree(d->fg_in);
  if (d->h_cnt) (void)hipHostFree(d->h_cnt);
  if (d->h_flagged) (void)hipHostFree(d->h_flagged);
  for (int i = 0; i < 2; ++i) {
    if (d->h_stargs[i]) (void)hipHostFree(d->h_stargs[i]);
    if (d->ev_stargs[i]) (void)hipEventDestroy(d->ev_stargs[i]);
  }
  for (int i = 0; i < 2; ++i) {
    if (d->h_pkargs[i]) (void)hipHostFree(d->h_pkargs[i]);
    if (d->ev_pkargs[i]) (void)hipEventDestroy(d->ev_pkargs[i]);
  }
  d->peek_args.release(); d->peek_status.release();
  d->cp_scratch.release();
  if (d->h_cp) (void)hipHostFree(d->h_cp);
  d->sk_rows.release(); d->sk_kept.release(); d->sk_lsm.release();
  d->al_bp.release(); d->al_lsm.release(); d->po_alpha.release(); d->gr_frames.release(); d->gs_args.release(); d->ed_bp.release();
  for (int i = 0; i < 2; ++i) {
    if (d->h_gsargs[i]) (void)hipHostFree(d->h_gsargs[i]);
    if (d->ev_gsargs[i]) (void)hipEventDestroy(d->ev_gsargs[i]);
  }
  if (d->h_sk) (void)hipHostFree(d->h_sk);
  if (d->ev_sk_tab) (void)hipEventDestroy(d->ev_sk_tab);
  for (int i = 0; i < 4; ++i) if (d->ev_sk[i]) (void)hipEventDestroy(d->ev_sk[i]);
  if (d->copy_stream) (void)hipStreamDestroy(d->copy_stream);
  if (d->ev_in) (void)hipEventDestroy(d->ev_in);
  if (d->ev_order) (void)hipEventDestroy(d->ev_order);
  if (d->ev0) { (void)hipEventDestroy(d->ev0); (void)hipEventDestroy(d->ev1); (void)hipEventDestroy(d->ev2); (void)hipEventDestroy(d->ev3); }
  d->pool.release(); d->status.release(); d->prof.release(); d->tables.release(); d->logp.release(); d->lsm.release(); d->pr_ml.release(); d->flags.release();
  d->stage_in.release(); d->stage_out.release(); d->pr_cnt.release(); d->pr_ch.release(); d->pr_lp.release(); d->far.release(); d->st_args.release(); d->prune_in.release(); d->prune_out.release(); d->st_lens.release();
  d->dbg.release(); d->tl.release();
  d->cb_blocks.release(); d->cb_ctl.release(); d->order.release();
  if (d->h_cb) (void)hipHostFree(d->h_cb);
  d->c_hdr.release(); d->c_ent.release(); d->c_rag.release(); d->c_cnt.release(); d->c_sc.release(); d->c_ln.release();
  if (d->h_stage) (void)hipHostFree(d->h_stage);
  delete d->workers;
  delete d;
}

int ctcd_debug_set_host_path(ctcd_decoder *d, int input_streaming, long long mirror_cap_labels) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  if (input_streaming >= 0) d->no_input_streaming = input_streaming == 0;
  d->stall_input_test = input_streaming == 2;  // tests: the rows are sent but "frames arrived" never advances -- the kernel must give up
  if (mirror_cap_labels >= -1) d->mirror_cap_override = mirror_cap_labels;
  return CTCD_OK;
}

// Forced alignment (align.hip): the budget of its back-pointer scratch, and the workgroups its last call launched.
int ctcd_set_align_scratch(ctcd_decoder *d, long long bytes) {
  if (!d || bytes < 0) return fail(CTCD_EINVAL, "ctcd_set_align_scratch: a decoder and bytes >= 0 (0 = the default) required");
  d->al_budget = bytes;
  return CTCD_OK;
}
long long ctcd_last_align_grid(const ctcd_decoder *d) { return d ? d->al_grid : -1; }

// CTC log-likelihood (loglik.hip): the cap of its grid, and the widest grid its last call launched.
int ctcd_set_loglik_grid(ctcd_decoder *d, long long max_workgroups) {
  if (!d || max_workgroups < 0) return fail(CTCD_EINVAL, "ctcd_set_loglik_grid: a decoder and max_workgroups >= 0 (0 = the default) required");
  d->ll_cap = max_workgroups;
  return CTCD_OK;
}
long long ctcd_last_loglik_grid(const ctcd_decoder *d) { return d ? d->ll_grid : -1; }

// Label posteriors (posterior.hip): the budget of the scratch that keeps the forward values, and the workgroups its last call launched.
int ctcd_set_posterior_scratch(ctcd_decoder *d, long long bytes) {
  if (!d || bytes < 0) return fail(CTCD_EINVAL, "ctcd_set_posterior_scratch: a decoder and bytes >= 0 (0 = the default) required");
  d->po_budget = bytes;
  return CTCD_OK;
}
long long ctcd_last_posterior_grid(const ctcd_decoder *d) { return d ? d->po_grid : -1; }

// Edit distance (editdist.hip): the pairs its last call ran.
long long ctcd_last_edit_pairs(const ctcd_decoder *d) { return d ? d->ed_pairs : -1; }
int ctcd_set_edit_grid(ctcd_decoder *d, long long max_workgroups) {
  if (!d || max_workgroups < 0) return fail(CTCD_EINVAL, "ctcd_set_edit_grid: a decoder and max_workgroups >= 0 (0 = the default) required");
  d->ed_cap = max_workgroups;
  return CTCD_OK;
}
long long ctcd_last_edit_grid(const ctcd_decoder *d) { return d ? d->ed_grid : -1; }
// Edit operations (editops.hip): the budget of ctcd_edit_align's back-pointer scratch, and the slots its last call used.
int ctcd_set_edit_scratch(ctcd_decoder *d, long long bytes) {
  if (!d || bytes < 0) return fail(CTCD_EINVAL, "ctcd_set_edit_scratch: a decoder and bytes >= 0 (0 = the default) required");
  d->ed_budget = bytes;
  return CTCD_OK;
}
long long ctcd_last_edit_slots(const ctcd_decoder *d) { return d ? d->ed_slots : -1; }

int ctcd_set_cu_sharing(ctcd_decoder *d, int mode) {
  if (!d || mode < -1 || mode > 1) return fail(CTCD_EINVAL, "cu sharing mode must be -1 (automatic), 0 or 1");
  d->cu_sharing = mode;
  return CTCD_OK;
}

int ctcd_set_exact_shape(ctcd_decoder *d, int mode) {
  if (!d || mode < -1 || mode > 1) return fail(CTCD_EINVAL, "exact shape mode must be -1 (automatic), 0 or 1");
  d->exact_shape = mode;
  return CTCD_OK;
}
int ctcd_last_exact_shape(const ctcd_decoder *d) { return d ? d->last_exact : -1; }

int ctcd_set_launch_order(ctcd_decoder *d, int mode) {
  if (!d || (mode != CTCD_ORDER_BATCH && mode != CTCD_ORDER_LENGTH)) return fail(CTCD_EINVAL, "launch order must be CTCD_ORDER_BATCH or CTCD_ORDER_LENGTH");
  d->launch_order = mode;
  return CTCD_OK;
}

int ctcd_debug_last_launch_order(ctcd_decoder *d, int32_t *out, int B) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  std::lock_guard<std::mutex> lock(d->mu);
  if (d->last_order_items == 0) return 0;
  if (!out || B != d->last_order_items)
    return fail(CTCD_EINVAL, "the last call's launch order has " + std::to_string(d->last_order_items) + " items");
  CTC_ON_DEVICE(d->device);
  // (the event behind the order pass: the caller's stream may be gone by now)
  HIP_TRY(hipEventSynchronize(d->ev_order));
  HIP_TRY(hipMemcpy(out, (char *)d->order.p + 4, (size_t)B * 4, hipMemcpyDeviceToHost));
  return 1;
}

int ctcd_set_subtree_search(ctcd_decoder *d, int mode) {
  if (!d || mode < -1 || mode > 1) return fail(CTCD_EINVAL, "subtree search mode must be -1 (automatic), 0 or 1");
  d->subtree_mode = mode;
  return CTCD_OK;
}
// (all three read the key of the last launch: recorded once it is queued)
int ctcd_last_subtree_search(const ctcd_decoder *d) {
  return d ? (d->last_kernel && (d->last_kernel->key.prof == 3 || d->last_kernel->key.prof == 5)) : -1;
}
int ctcd_debug_last_layout(const ctcd_decoder *d) { return d && d->last_kernel ? layout_of(d->last_kernel->key) : -1; }
int ctcd_debug_last_kernel(const ctcd_decoder *d, int32_t params[7]) {
  if (!d || !params) return fail(CTCD_EINVAL, "decoder == NULL or params == NULL");
  if (!d->last_kernel) return CTCD_EINVAL;  // (no launch yet: ctcd_last_error is left as it was)
  const KernelKey &k = d->last_kernel->key;
  const int32_t p[7] = {k.prof, k.big, k.layout, k.pruned, k.nt, k.lm, k.occ2};
  std::memcpy(params, p, sizeof(p));
  return CTCD_OK;
}

int ctcd_set_input_dtype(ctcd_decoder *d, int dtype) {
  if (!d || (dtype != CTCD_DTYPE_F32 && dtype != CTCD_DTYPE_F16 && dtype != CTCD_DTYPE_BF16))
    return fail(CTCD_EINVAL, "dtype must be CTCD_DTYPE_F32, CTCD_DTYPE_F16 or CTCD_DTYPE_BF16");
  d->in_dtype = dtype;
  return CTCD_OK;
}
int ctcd_last_input_dtype(ctcd_decoder *d) { return d ? d->last_in_dtype : -1; }

int ctcd_set_threads(ctcd_decoder *d, int t) {
  if (!d || t < 0 || t > 1024 || (t && (t < 64 || (t & (t - 1))))) return fail(CTCD_EINVAL, "threads must be 0 (automatic) or a power of two in [64, 1024]");
  d->threads = t;
  return CTCD_OK;
}

// ---- the pre-pass launches (kernels, and the table they are picked from: prepass.h)
// The tables of the bit-exact float32 exp / log (exact_math.h) on the device, uploaded by the first call that needs them.  (The
// caller holds d->mu.)
static int ensure_tables(ctcd_decoder *d) {
  if (d->tables_ready) return CTCD_OK;
  if (int rc = d->tables.ensure(sizeof(ctcmath::Tables))) return rc;
  HIP_TRY(hipMemcpy(d->tables.p, ctcmath::host_tables().w, sizeof(ctcmath::Tables), hipMemcpyHostToDevice));
  d->tables_ready = true;
  return CTCD_OK;
}

// the element size of an input dtype
static size_t in_elem_bytes(int dt) { return dt == CTCD_DTYPE_F32 ? 4 : 2; }
// Rows of V elements of dtype `dt` from this base take the bandwidth-shaped workgroup kernels, which read four elements per load (the
// base 16-byte aligned for float32 rows, 8-byte for half rows).  Each dispatch site adds its own conditions.
static bool takes_load4(int V, const void *rows, int dt) {
  return V % 4 == 0 && V > 256 && V <= 16384 && ((uintptr_t)rows & (4 * in_elem_bytes(dt) - 1)) == 0;
}

// log_softmax of every frame (ctcd_log_softmax's definition): long rows by a workgroup each, short ones by a wave each
static int launch_log_softmax(ctcd_decoder *d, const float *in, float *out, long long rows, const int32_t *lens, int T, int V, hipStream_t stream,
                              int dt = CTCD_DTYPE_F32) {
  if (dt != CTCD_DTYPE_F16 && dt != CTCD_DTYPE_BF16) dt = CTCD_DTYPE_F32;
  const uint64_t *tb = (const uint64_t *)d->tables.p;
  void *args[] = {(void *)&in, (void *)&out, (void *)&rows, (void *)&lens, (void *)&T, (void *)&V, (void *)&tb};
  if (takes_load4(V, in, dt) && ((uintptr_t)out & 15) == 0 && !d->no_fused_logits) {
    const void *fn = pp_pick(CTCD_PP_LSM_WG, 0, dt, V)->fn;
    const dim3 grid((unsigned)std::min<long long>(rows, 256 * 32));
    HIP_TRY(hipLaunchKernel(fn, grid, dim3(256), args, 0, stream));
    d->pre_fn[1] = fn;
  } else {
    const void *fn = pp_pick(CTCD_PP_LSM_WAVE, 0, dt, 0)->fn;
    HIP_TRY(hipLaunchKernel(fn, dim3((unsigned)std::min<long long>((rows + 3) / 4, 256 * 64)), dim3(256), args, 0, stream));
    d->pre_fn[1] = fn;
  }
  HIP_TRY(hipGetLastError());
  return CTCD_OK;
}

// The elementwise pre-passes into the decoder's workspace: prob -> log (to_log), or half rows widened as they are.
static int launch_elementwise(ctcd_decoder *d, const float *in, float *out, size_t n, const int32_t *lens, int T, int V, hipStream_t stream, int dt,
                              bool to_log) {
  const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
  const PrepassEntry *e = pp_pick(to_log ? CTCD_PP_PROB_TO_LOG : CTCD_PP_WIDEN, 0, dt, V);
  if (!e) return fail(CTCD_EINTERNAL, "no elementwise pre-pass for this input dtype");
  const void *fn = e->fn;
  void *args[] = {(void *)&in, (void *)&out, (void *)&n, (void *)&lens, (void *)&T, (void *)&V};
  HIP_TRY(hipLaunchKernel(fn, dim3(blocks), dim3(256), args, 0, stream));
  HIP_TRY(hipGetLastError());
  d->pre_fn[0] = fn;
  return CTCD_OK;
}

// The vocabulary-prune kernels for one input dtype (decode_common picks among them by shape)
struct PruneFns { const void *rows, *wg, *wg_reg, *logits, *resolve; };
static PruneFns prune_fns(int dt, int V) {
  PruneFns f;
  f.rows = pp_pick(CTCD_PP_PRUNE_ROWS, 0, dt, V)->fn;
  f.wg = pp_pick(CTCD_PP_PRUNE_WG, 0, dt, V)->fn;
  const PrepassEntry *reg = pp_pick(CTCD_PP_PRUNE_WG, 1, dt, V);  // (none beyond 10240 labels: the two-sweep form)
  f.wg_reg = reg ? reg->fn : f.wg;
  f.logits = pp_pick(CTCD_PP_PRUNE_LOGITS, 0, dt, V)->fn;
  f.resolve = pp_pick(CTCD_PP_RESOLVE, 0, dt, V)->fn;
  return f;
}

// The vocabulary prune of every frame of a call (it also converts the kept probabilities to log space when log_input == 0), and the
// settling of the frames it flags, queued on `stream`: d->pr_cnt / pr_ch / pr_lp hold each frame's kept labels (`stride` per frame)
// for the decode kernel.  fuse_logits: the rows are raw logits and prune_logits_wg_kernel normalises them as it reads them.
static int launch_prune(ctcd_decoder *d, const float *probs, const int32_t *pre_lens, int B, int T, int V, int stride, double cutoff_prob,
                        int cutoff_top_n, int log_input, int dt, bool fuse_logits, hipStream_t stream) {
  int rc;
  const long long rows = (long long)B * T;

  if ((rc = d->pr_cnt.ensure((size_t)rows * 4))) return rc;
  if ((rc = d->pr_ch.ensure((size_t)rows * stride * 4))) return rc;
  if ((rc = d->pr_lp.ensure((size_t)rows * stride * 4))) return rc;
  const int wpb = 4;
  const size_t psm = (size_t)wpb * (3 * (size_t)stride + 2 * kPruneCand) * 4;
  if (psm > (size_t)d->max_lds) return fail(CTCD_EUNSUPPORTED, "cutoff_top_n too large for the prune pass");
  const int blocks = (int)std::min<long long>((rows + wpb - 1) / wpb, 256 * 16);
  const PruneFns fns = prune_fns(dt, V);
  const void *pfn = fns.rows;
  bool wg_kernel = false;
  // the bandwidth-shaped variant
  if (takes_load4(V, probs, dt) && std::min(cutoff_top_n, V) <= 64) {
    wg_kernel = true;
    pfn = fns.wg;
    static const bool reg_rows = getenv("CTCD_PRUNE_REG") ? atoi(getenv("CTCD_PRUNE_REG")) != 0 : true;
    if (reg_rows && !d->no_prune_reg) pfn = fns.wg_reg;  // the row held in registers between the two looks at it
  }
  if (fuse_logits) {  // (same shape conditions)
    pfn = fns.logits;
    if ((rc = d->pr_ml.ensure((size_t)rows * 8))) return rc;
  }
  const size_t psm_launch = wg_kernel ? (3 * (size_t)stride + 3 * kPruneCand + 4) * 4 : psm;
  // (measured: a persistent grid of 1280 or 2560 workgroups is slower, 16 k / 32 k the same)
  const int blocks_launch = wg_kernel ? (int)std::min<long long>(rows, 256 * 32) : blocks;
  HIP_TRY(hipFuncSetAttribute(pfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)psm_launch));
  // Frames the fast pass cannot settle (ties at the cut, a cumulative sum next to cutoff_prob) are flagged and settled by
  // prune_resolve_kernel right behind it -- on the device, on the same stream: no read-back, no host arithmetic, no
  // synchronisation before the decode kernel.  The flag list holds every frame of the call (rows words).
  const unsigned cap = (unsigned)std::min<long long>(rows, 0x7fffffffLL);
  if ((rc = d->flags.ensure(8 + (size_t)cap * 4))) return rc;
  unsigned *n_flag = (unsigned *)d->flags.p, *flag_rows = (unsigned *)((char *)d->flags.p + 8);
  d->prune_timed = false;
  const size_t rbytes = prune_resolve_lds_bytes(V, std::min(cutoff_top_n, V));
  const bool in_lds = rbytes + 1024 <= (size_t)d->max_lds && !d->resolve_in_global;
  const int rblocks = in_lds ? 256 : 64;
  if (in_lds) HIP_TRY(hipFuncSetAttribute(fns.resolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rbytes));
  const size_t rstride = (rbytes + 255) / 256 * 256;
  if (!in_lds && (rc = d->prune_in.ensure(rstride * rblocks))) return rc;  // (rows too long for LDS: the sort's arrays in global memory)
  HIP_TRY(hipMemsetAsync(n_flag, 0, 8, stream));
  HIP_TRY(hipMemsetAsync(d->pr_cnt.p, 0, (size_t)rows * 4, stream));
  PruneArgs pa;
  pa.in = probs; pa.seq_lens = pre_lens; pa.T = T; pa.V = V; pa.top_n = cutoff_top_n; pa.log_input = log_input;
  pa.stride = stride; pa.rows = rows; pa.cutoff_prob = cutoff_prob; pa.cnt = (int *)d->pr_cnt.p; pa.ch = (int *)d->pr_ch.p;
  pa.lp = (float *)d->pr_lp.p; pa.n_flag = n_flag; pa.flag_rows = flag_rows; pa.flag_cap = cap;
  pa.cut_exp = std::exp(cutoff_prob); pa.tables = (const uint64_t *)d->tables.p;
  pa.row_max = fuse_logits ? (float *)d->pr_ml.p : nullptr; pa.row_lse = fuse_logits ? (float *)d->pr_ml.p + rows : nullptr;
  const uint64_t *ptables = (const uint64_t *)d->tables.p;
  void *pargs[] = {&pa, (void *)&ptables};  // (the second argument: prune_logits_wg_kernel only)
  if (d->timing) HIP_TRY(hipEventRecord(d->ev2, stream));
  HIP_TRY(hipLaunchKernel(pfn, dim3(blocks_launch), dim3(wpb * 64), pargs, psm_launch, stream));
  HIP_TRY(hipGetLastError());
  d->pre_fn[2] = pfn;
  if (d->timing) { HIP_TRY(hipEventRecord(d->ev3, stream)); d->prune_timed = true; }
  // (prune_resolve_kernel keeps positions and counters in 16 bits: the refusal of pruning with more than 32767 labels above is
  //  what guarantees they fit -- said here, next to the launch, so that the two cannot drift apart: ADVICE r4)
  static_assert(kResolveMaxV >= 32767, "prune_resolve_kernel's 16-bit positions must cover every vocabulary the prune pass accepts");
  if (V > kResolveMaxV) return fail(CTCD_EUNSUPPORTED, "vocabulary pruning: too many labels for the std::sort replay's 16-bit positions");
  char *rfar = in_lds ? (char *)nullptr : (char *)d->prune_in.p;
  size_t rstride_arg = rstride;
  void *rargs[] = {&pa, (void *)&rfar, (void *)&rstride_arg};
  HIP_TRY(hipLaunchKernel(fns.resolve, dim3(rblocks), dim3(kResolveThreads), rargs, in_lds ? rbytes : 0, stream));
  HIP_TRY(hipGetLastError());
  d->pre_fn[3] = fns.resolve;
  d->pre_resolve_global = !in_lds;
  // (statistics only: the number of flagged frames travels to page-locked memory behind the kernels; whoever asks for it
  //  -- ctcd_last_prune_flagged_rows -- waits for the stream)
  if (!d->h_flagged) HIP_TRY(hipHostMalloc((void **)&d->h_flagged, 8, hipHostMallocDefault));
  HIP_TRY(hipMemcpyAsync(d->h_flagged, n_flag, 4, hipMemcpyDeviceToHost, stream));
  d->flagged_pending = true;
  return CTCD_OK;
}

// What the last call's pre-passes launched, read back from the launched pointers through kPrepass: four stages of {kernel, a, b, dt}.
int ctcd_debug_last_prepass(const ctcd_decoder *d, int32_t out[CTCD_PREPASS_FIELDS]) {
  if (!d || !out) return fail(CTCD_EINVAL, "decoder == NULL or out == NULL");
  for (int s = 0; s < 4; ++s) {
    int32_t *o = out + 4 * s;
    o[0] = o[1] = o[2] = o[3] = 0;
    if (!d->pre_fn[s]) continue;
    const PrepassEntry *e = pp_find(d->pre_fn[s]);
    if (!e) return fail(CTCD_EINTERNAL, "the last call launched a pre-pass kernel that is not in the table");
    o[0] = e->kernel; o[1] = e->a; o[2] = s == 3 ? (d->pre_resolve_global ? 1 : 0) : e->b; o[3] = e->dt;
  }
  return CTCD_OK;
}
int ctcd_debug_prepass_table(int32_t *out, int cap) {
  const int n = kPrepassCount;
  for (int i = 0; out && i < n && i < cap; ++i) {
    const PrepassEntry &e = kPrepass[i];
    int32_t *o = out + 5 * i;
    o[0] = e.kernel; o[1] = e.a; o[2] = e.b; o[3] = e.dt; o[4] = e.vmax;
  }
  return n;
}

static int decode_common(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                         double cutoff_prob, int cutoff_top_n, int blank_id, int log_input, int32_t *out_tok, int32_t *out_ts,
                         float *out_sc, int32_t *out_len, int32_t *n_results, void *stream_, const StreamCall *sc,
                         ctcd_scorer *scorer = nullptr, const CompactOut *co = nullptr, const int *frames_ready = nullptr) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  if (scorer && scorer->device != d->device) return fail(CTCD_EINVAL, "the scorer's tables live on another device than the decoder");
  if (scorer && (int)scorer->host.labels.size() != V) return fail(CTCD_EINVAL, "the scorer was built for a different number of labels");
  const int out_T = sc ? sc->out_T : T;
  // (a streaming call in which no stream ends has out_T == 0 and may pass null token / timestep buffers)
  const bool no_rows = (sc && out_T == 0) || co;
  if (co && (out_T > 65536 || V > 65535)) return fail(CTCD_EUNSUPPORTED, "compact results pack label and frame into 16 bits each");
  int rc = check_args(B, T, V, beam, cutoff_top_n, blank_id, probs, no_rows ? (const void *)d : (const void *)out_tok,
                      no_rows ? (const void *)d : (const void *)out_ts, out_sc, out_len);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(d->mu);
  hipStream_t stream = (hipStream_t)stream_;
  CTC_ON_DEVICE(d->device);
  if (B == 0) {
    if (!sc) d->last_order_items = 0;  // (ctcd_debug_last_launch_order: an empty call has no order)
    return CTCD_OK;
  }
  cutoff_prob = used_cutoff_prob(cutoff_prob);  // (from here on, < 1.0 <=> the reference's cumulative cut)
  const Dims dims = make_dims(beam, V, cutoff_top_n, cutoff_prob, scorer != nullptr);
  // the kernel, its workgroup size and its LDS, before anything is queued: a call this build refuses leaves no trace
  const ScorerKind sk = !scorer ? kNoScorer : scorer->cbl ? kCallbackScorer
                        : (!scorer->host.char_based && !scorer->host.dict_wide && !d->general_lm_kernel) ? kWordScorer : kGeneralScorer;
  const LaunchSwitches sw{d->no_fixed_layout, d->profile, d->tl_armed, d->cu_sharing, d->subtree_mode, d->subtree_on};
  const LaunchPlan plan = plan_launch(dims, B, d->threads, d->max_lds, d->cu_count, sw, sk, frames_ready != nullptr,
                                      [](const KernelKey &k) { return kernel_entry(k) != nullptr; });
  if (plan.rc) return fail(plan.rc, plan.msg);
  const KernelEntry *kernel = kernel_entry(plan.key);  // (plan_launch plans only what the build's list holds)
  // an exact-shape twin in the planned kernel's place (same workgroup, same workspace, same arguments); the record of the launch --
  // ctcd_debug_last_* -- stays the planned key
  const ExactEntry *exact = d->exact_shape != 0 ? exact_entry(plan.key, dims, blank_id, !sc && !frames_ready) : nullptr;
  if (d->exact_shape == 1 && !exact)
    return fail(CTCD_EUNSUPPORTED, "ctcd_set_exact_shape(1): this call does not qualify for an exact-shape kernel (decode_kernel.h CTC_EXACT_SHAPES)");
  const void *kernel_fn = exact ? exact->fn : kernel->fn;
  const int threads = plan.threads;
  size_t lds = plan.lds;
  const size_t far_bytes = plan.far_bytes;
  if ((rc = d->far.ensure((size_t)B * far_bytes))) return rc;

  // outputs: everything outside the valid region is defined as 0
  const size_t kt = co ? 0 : (size_t)B * beam * out_T;
  if (co && !(sc && sc->no_clear)) {  // (resumed launches of the scorer hook: the records of items that finished earlier stay)
    HIP_TRY(hipMemsetAsync(co->count, 0, 4, stream));
    HIP_TRY(hipMemsetAsync(co->hdr, 0, (size_t)B * 16, stream));
  }
  if (kt && !(sc && sc->no_clear)) {
    HIP_TRY(hipMemsetAsync(out_tok, 0, kt * 4, stream));
    HIP_TRY(hipMemsetAsync(out_ts, 0, kt * 4, stream));
  }
  if ((!sc || sc->any_eos) && !(sc && sc->no_clear)) {  // (a streaming call in which no stream ends writes no results: nothing to define)
    HIP_TRY(hipMemsetAsync(out_sc, 0, (size_t)B * beam * 4, stream));
    HIP_TRY(hipMemsetAsync(out_len, 0, (size_t)B * beam * 4, stream));
    if (sc && n_results) HIP_TRY(hipMemsetAsync(n_results, 0, (size_t)B * 4, stream));
  }

  if ((rc = ensure_tables(d))) return rc;
  // streaming: per-item block pointers, pool capacities and end-of-stream flags go to the device
  char **st_base = nullptr;
  int *st_cap = nullptr;
  unsigned char *st_eos = nullptr;
  if (sc) {
    // [block pointers | pool capacities | chunk lengths | end-of-stream flags], staged in page-locked memory (two slots,
    // an event each) and sent with ONE asynchronous copy: a chunk call synchronises nothing (round 3: two stream
    // synchronisations per call, one for this block and one for the lengths)
    const size_t off_cap = (size_t)B * 8, off_len = off_cap + (size_t)B * 4, off_eos = off_len + (size_t)B * 4, need = (off_eos + (size_t)B + 31) & ~(size_t)15;
    if ((rc = d->st_args.ensure(2 * need))) return rc;
    if (d->h_stargs_cap < need) {
      for (int i = 0; i < 2; ++i) {
        if (d->ev_stargs[i]) HIP_TRY(hipEventSynchronize(d->ev_stargs[i]));
        if (d->h_stargs[i]) (void)hipHostFree(d->h_stargs[i]);
        d->h_stargs[i] = nullptr;
        HIP_TRY(hipHostMalloc((void **)&d->h_stargs[i], need, hipHostMallocDefault));
        if (!d->ev_stargs[i]) HIP_TRY(hipEventCreateWithFlags(&d->ev_stargs[i], hipEventDisableTiming));
      }
      d->h_stargs_cap = need;
    }
    const int slot = (int)(d->stream_calls++ & 1);
    HIP_TRY(hipEventSynchronize(d->ev_stargs[slot]));  // (the copy of two calls ago: long done)
    char *hb = d->h_stargs[slot];
    for (int b = 0; b < B; ++b) {
      ctcd_stream *st = sc->states[b];
      ((char **)hb)[b] = st->block;
      ((int *)(hb + off_cap))[b] = (int)(st->cap_frames * beam + 1);
      ((int *)(hb + off_len))[b] = sc->lens[b];
      hb[off_eos + b] = sc->is_eos[b] ? 1 : 0;
    }
    char *db = (char *)d->st_args.p + (size_t)slot * need;
    HIP_TRY(hipMemcpyAsync(db, hb, off_eos + (size_t)B, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(d->ev_stargs[slot], stream));
    st_base = (char **)db;
    st_cap = (int *)(db + off_cap);
    st_eos = (unsigned char *)db + off_eos;
    seq_lens = (const int32_t *)(db + off_len);
  }
  // ctcd_debug_last_prepass: what this call's pre-passes launch, recorded as each is queued
  std::fill(d->pre_fn, d->pre_fn + 4, nullptr);
  // the rows the pre-passes cover (resumed launches of the scorer hook start inside the rows: StreamCall::row_lens)
  const int32_t *pre_lens = (sc && sc->row_lens) ? sc->row_lens : seq_lens;
  // half rows (ctcd_set_input_dtype): the pre-pass kernels read them; `probs` keeps pointing at the caller's rows until a pass has
  // written float32 rows into the workspace (dt = kInF32 from there on).  The decode kernels themselves only ever read float32.
  int dt = (sc && sc->in_dtype >= 0) ? sc->in_dtype : d->in_dtype;
  d->last_in_dtype = dt;
  if (dt != CTCD_DTYPE_F32 && scorer && log_input != 2 && T > 0) {
    // the LM tier reads the blank's value from the caller's rows (KernelArgs::raw): one widening pass into the workspace, then the
    // float32 route (raw logits are normalised into the workspace below anyway)
    if ((rc = d->lsm.ensure((size_t)B * T * V * 4))) return rc;
    if (pre_lens) HIP_TRY(hipMemsetAsync(d->lsm.p, 0, (size_t)B * T * V * 4, stream));
    if ((rc = launch_elementwise(d, probs, (float *)d->lsm.p, (size_t)B * T * V, pre_lens, T, V, stream, dt, false))) return rc;
    probs = (const float *)d->lsm.p;
    dt = CTCD_DTYPE_F32;
  }

  // raw logits in front of a vocabulary prune: one pass does both (prune_logits_wg_kernel -- the normalised rows are never written).
  // Not with a scorer: the LM tier reads the blank's log-probability from the rows themselves (ctc_beam_search_decoder.cpp:78).
  const bool fuse_logits = log_input == 2 && dims.use_rank_table && T > 0 && !scorer && !d->no_fused_logits && std::min(cutoff_top_n, V) <= 64 &&
                           takes_load4(V, probs, dt);
  if (log_input == 2 && !fuse_logits) {  // raw logits: normalise once, in HBM; everything below sees log-probabilities
    if (T > 0) {
      if ((rc = d->lsm.ensure((size_t)B * T * V * 4))) return rc;
      if (pre_lens) HIP_TRY(hipMemsetAsync(d->lsm.p, 0, (size_t)B * T * V * 4, stream));  // frames past an utterance's end stay defined
      if ((rc = launch_log_softmax(d, probs, (float *)d->lsm.p, (long long)B * T, pre_lens, T, V, stream, dt))) return rc;
      probs = (const float *)d->lsm.p;
      dt = CTCD_DTYPE_F32;
    }
    log_input = 1;
  }
  const long long pool_stride = (long long)beam * T + 1;
  // per utterance: nodes (12 B each), then -- per utterance again -- express pointers and the time steps' high parts (4 B each)
  if (!sc && (rc = d->pool.ensure((size_t)B * pool_stride * (sizeof(PoolNode) + 2 * sizeof(int))))) return rc;
  if ((rc = d->status.ensure((size_t)B * 8))) return rc;  // [status words | beam-shape statistic]
  // every status word starts as -1 ("no result"): a workgroup that never ran cannot read back as ST_OK
  HIP_TRY(hipMemsetAsync(d->status.p, 0xff, (size_t)B * 4, stream));
  d->last_stream = stream;
  const float *logp = probs;
  d->prune_flagged_rows = 0;
  d->flagged_pending = false;
  if (dims.use_rank_table && T > 0) {
    // vocabulary prune pass (also converts the kept probabilities to log space when log_input == 0)
    if ((rc = launch_prune(d, probs, pre_lens, B, T, V, dims.Vc_max, cutoff_prob, cutoff_top_n, log_input, dt, fuse_logits, stream))) return rc;
  } else if ((!log_input || dt != CTCD_DTYPE_F32) && T > 0) {
    // probabilities -> log-probabilities, or half log-probability rows widened: the decode kernel reads float32 rows
    const size_t n = (size_t)B * T * V;
    if ((rc = d->logp.ensure(n * 4))) return rc;
    if (pre_lens) HIP_TRY(hipMemsetAsync(d->logp.p, 0, n * 4, stream));  // frames past an utterance's end stay defined
    if ((rc = launch_elementwise(d, probs, (float *)d->logp.p, n, pre_lens, T, V, stream, dt, !log_input))) return rc;
    logp = (const float *)d->logp.p;
  }

  KernelArgs a;
  a.probs = logp; a.seq_lens = seq_lens; a.B = B; a.T = T; a.V = V; a.K = beam; a.blank = blank_id; a.dims = dims;
  a.pool = (PoolNode *)d->pool.p; a.pool_stride = pool_stride;
  a.pool_up = (int *)(a.pool + (size_t)B * pool_stride);
  a.tables = (const uint64_t *)d->tables.p;
  a.outs.tok = out_tok; a.outs.ts = out_ts; a.outs.len = out_len; a.outs.n_results = n_results; a.outs.score = out_sc;
  a.outs.K = beam; a.outs.T_stride = out_T;
  a.outs.c_hdr = nullptr; a.outs.c_ent = nullptr; a.outs.c_rag = nullptr; a.outs.c_count = nullptr; a.outs.c_cap = 0;
  a.outs.m_hdr = nullptr; a.outs.m_ent = nullptr; a.outs.m_done = nullptr; a.outs.m_rag = nullptr; a.outs.m_cap = 0;
  if (co) {
    a.outs.tok = nullptr; a.outs.ts = nullptr;
    a.outs.c_hdr = co->hdr; a.outs.c_ent = co->ent; a.outs.c_rag = co->rag; a.outs.c_count = co->count; a.outs.c_cap = co->cap;
    a.outs.m_hdr = co->m_hdr; a.outs.m_ent = co->m_ent; a.outs.m_done = co->m_done; a.outs.m_rag = co->m_rag; a.outs.m_cap = co->m_cap;
  }
  a.status = (int32_t *)d->status.p;
  a.shape = a.status + B;
  d->status_items = B;
  a.st_base = st_base; a.st_poolcap = st_cap; a.st_eos = st_eos; a.st_pool_off = (long long)stream_pool_offset(beam);
  a.raw = probs; a.raw_log = log_input;
  std::memset(&a.lm, 0, sizeof(a.lm));
  if (scorer) {
    a.lm = scorer->dview;
    a.lm.alpha = scorer->host.alpha;  // reset_params (binding.cpp:283-287) takes effect at the next decode
    a.lm.beta = scorer->host.beta;
  }
  a.frames_ready = frames_ready;  // (streamed input of the host-tensor entry point; null: every row is in place)
  a.cb_log_len = nullptr; a.cb_log_idx = nullptr; a.cb_log_slot = nullptr; a.cb_done = nullptr; a.cb_ans = nullptr;
  a.lm.cb_ring = 0;
  if (sc && sc->live) {
    a.lm.cb_ring = 1;
    a.cb_log_len = (const unsigned *)sc->live; a.cb_done = (int32_t *)(sc->live + kLiveOffDone); a.cb_ans = (const unsigned *)(sc->live + kLiveOffAns);
    a.cb_log_idx = (const uint32_t *)(sc->live + kLiveOffIdx); a.cb_log_slot = (const ctclm::NgSlot *)(sc->live + kLiveOffSlot);
  }
  a.frame_off = sc ? sc->frame_off : nullptr;
  a.frames_done = sc ? sc->frames_done : nullptr;
  a.pr_cnt = nullptr; a.pr_ch = nullptr; a.pr_lp = nullptr; a.pr_stride = 0;
  if (dims.use_rank_table) {
    a.pr_cnt = (const int *)d->pr_cnt.p; a.pr_ch = (const int *)d->pr_ch.p; a.pr_lp = (const float *)d->pr_lp.p;
    a.pr_stride = dims.Vc_max;
  }
  a.prof = nullptr;
  a.dbg = nullptr;
  a.tl = nullptr; a.tl_cap = kTimelineCap; a.tl_f0 = d->tl_f0; a.tl_nf = d->tl_nf;
  if (d->profile && d->tl_armed) {
    if ((rc = d->tl.ensure((size_t)16 * kTimelineCap * 8))) return rc;
    HIP_TRY(hipMemsetAsync(d->tl.p, 0, (size_t)16 * kTimelineCap * 8, stream));
    a.tl = (long long *)d->tl.p;
  }
  if (d->profile && d->dbg_on) {
    if ((rc = d->dbg.ensure((size_t)(T + 1) * (1 + 4 * (size_t)beam) * 4))) return rc;
    a.dbg = (int *)d->dbg.p;
  }
  if (d->profile) {
    if ((rc = d->prof.ensure((size_t)B * 16 * 8))) return rc;
    a.prof = (long long *)d->prof.p;
  }
  a.far = (char *)d->far.p; a.far_stride = (long long)far_bytes;
  // (CTCD_LDS_FLOOR: experiments with the occupancy the LDS request allows)
  if (d->lds_floor >= 0) lds = std::max(lds, std::min((size_t)d->lds_floor, (size_t)d->max_lds - 2048));
  HIP_TRY(hipFuncSetAttribute(kernel_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // launch order (ctcd_set_launch_order): the one-shot entry points, and every launch of a one-shot decode through a callback scorer
  // (a resumed launch by the frames each utterance has left; the debug copy shows the first launch's order); streaming calls keep
  // batch order.  The order pass runs on the same stream, from the lengths already on the device: nothing waits for the host.
  // (the wide-beam run-time layouts -- BIG kernels at LAYOUT 0 -- take no order: decode_kernel.h kTicket)
  const bool by_length = d->launch_order == CTCD_ORDER_LENGTH && (!sc || sc->one_shot) && takes_launch_order(plan.key);
  const bool first_launch = !sc || !sc->no_clear;
  const bool records = (!sc || sc->one_shot) && first_launch;  // (the launch ctcd_debug_last_launch_order reports)
  a.order = nullptr;
  if (by_length) {
    // [ticket | B items] of the first launch at 0, of a resumed launch (scorer hook) behind it
    const size_t region = ((size_t)B + 64) * 4;
    if ((rc = d->order.ensure(2 * region))) return rc;
    a.order = (int *)((char *)d->order.p + (first_launch ? 0 : region));
    if (records && !d->ev_order) HIP_TRY(hipEventCreateWithFlags(&d->ev_order, hipEventDisableTiming));
  }
  if (d->timing) HIP_TRY(hipEventRecord(d->ev0, stream));  // (with length order the timed span includes the order pass)
  if (by_length) {
    HIP_TRY(launch_order(seq_lens, B, T, d->max_lds, a.order, stream));
    if (records) HIP_TRY(hipEventRecord(d->ev_order, stream));
  }
  void *kargs[] = {&a};
  HIP_TRY(hipLaunchKernel(kernel_fn, dim3(B), dim3(threads), kargs, lds, stream));
  HIP_TRY(hipGetLastError());
  d->last_exact = exact ? 1 : 0;
  d->last_kernel = kernel;  // (recorded once the launch is queued: a launch that failed leaves the last record)
  if (d->timing) HIP_TRY(hipEventRecord(d->ev1, stream));
  if (records) d->last_order_items = by_length ? B : 0;  // (set once the launch is queued: a call that failed leaves the last record)
  return CTCD_OK;
}

int ctcd_beam_decode(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                     int /*num_processes*/, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                     int32_t *out_tok, int32_t *out_ts, float *out_sc, int32_t *out_len, int32_t *n_results, void *stream_) {
  return decode_common(d, probs, seq_lens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, out_tok, out_ts, out_sc,
                       out_len, n_results, stream_, nullptr);
}

// ---- LM tier: the external scorer (binding.cpp:122-150,263-287)
int ctcd_scorer_create(ctcd_scorer **out, double alpha, double beta, const char *lm_path, const char *const *labels, int V,
                       int device_id) {
  if (!out || !lm_path || !labels || V <= 0) return fail(CTCD_EINVAL, "bad scorer arguments");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail(CTCD_EINVAL, "no such HIP device");
  std::vector<std::string> lab(V);
  for (int i = 0; i < V; ++i) {
    if (!labels[i]) return fail(CTCD_EINVAL, "null label");
    lab[i] = labels[i];
  }
  ctcd_scorer *s = new ctcd_scorer;
  s->device = device_id;
  if (!s->host.build(alpha, beta, lm_path, lab)) {
    const std::string msg = s->host.error;
    delete s;
    return fail(msg.find("not supported") != std::string::npos || msg.find("supported for") != std::string::npos ? CTCD_EUNSUPPORTED : CTCD_EINVAL, msg);
  }
  CTC_ON_DEVICE(device_id);
  const ctclm::HostScorer &h = s->host;
  size_t off = 0;
  auto place = [&off](size_t bytes) { const size_t o = off; off = (off + bytes + 255) / 256 * 256; return o; };
  const size_t o_up = place(h.uni_prob.size() * 4), o_us = place(h.uni_state.size() * 4), o_bo = place(h.st_bo.size() * 4),
               o_fl = place(h.st_fail.size() * 4), o_ng = place(h.ng.size() * sizeof(ctclm::NgSlot)),
               o_dc = place(h.dict.size() * sizeof(ctclm::DictNode)), o_lw = place(h.label_word.size() * 4), o_dl = place(h.dict_lab.size() * 4);
  hipError_t e = hipMalloc((void **)&s->blob, off ? off : 256);
  if (e != hipSuccess) { delete s; return fail(CTCD_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  auto up = [&](size_t o, const void *src, size_t bytes) { return bytes ? hipMemcpy(s->blob + o, src, bytes, hipMemcpyHostToDevice) : hipSuccess; };
  if ((e = up(o_up, h.uni_prob.data(), h.uni_prob.size() * 4)) != hipSuccess || (e = up(o_us, h.uni_state.data(), h.uni_state.size() * 4)) != hipSuccess ||
      (e = up(o_bo, h.st_bo.data(), h.st_bo.size() * 4)) != hipSuccess || (e = up(o_fl, h.st_fail.data(), h.st_fail.size() * 4)) != hipSuccess ||
      (e = up(o_ng, h.ng.data(), h.ng.size() * sizeof(ctclm::NgSlot))) != hipSuccess ||
      (e = up(o_dc, h.dict.data(), h.dict.size() * sizeof(ctclm::DictNode))) != hipSuccess ||
      (e = up(o_lw, h.label_word.data(), h.label_word.size() * 4)) != hipSuccess ||
      (e = up(o_dl, h.dict_lab.data(), h.dict_lab.size() * 4)) != hipSuccess) {
    (void)hipFree(s->blob);
    delete s;
    return fail(CTCD_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  s->dview = h.view();
  s->dview.uni_prob = (const float *)(s->blob + o_up); s->dview.uni_state = (const uint32_t *)(s->blob + o_us);
  s->dview.st_bo = (const float *)(s->blob + o_bo); s->dview.st_fail = (const uint32_t *)(s->blob + o_fl);
  s->dview.ng = (const ctclm::NgSlot *)(s->blob + o_ng); s->dview.dict = (const ctclm::DictNode *)(s->blob + o_dc);
  s->dview.label_word = (const uint32_t *)(s->blob + o_lw);
  s->dview.dict_lab = (const uint32_t *)(s->blob + o_dl);
  s->fingerprint = ctcsnap::scorer_fingerprint(h);
  *out = s;
  return CTCD_OK;
}

void ctcd_scorer_destroy(ctcd_scorer *s) {
  if (!s) return;
  DeviceGuard guard_(s->device);
  if (s->blob) (void)hipFree(s->blob);
  for (char *p : {s->cb_ng, s->cb_st, s->cb_uni, s->cb_miss, s->cb_stage})
    if (p) (void)hipFree(p);
  if (s->h_live) (void)hipHostFree(s->h_live);
  if (s->cb_stage_hp) (void)hipHostFree(s->cb_stage_hp);
  if (s->cb_stage_ev) (void)hipEventDestroy(s->cb_stage_ev);
  s->ask_pool.shutdown();
  delete s->cbl;
  delete s;
}

// ---- the host-side scorer hook (binding.cpp:122-150 hands the decoder an opaque scorer; scorer.h:41-78 is its interface)
// Brings the device copy of the cache up to date with the host's: whole tables after a rehash / growth, single slots otherwise.
__global__ void cb_scatter_kernel(ctclm::NgSlot *ng, const uint32_t *idx, const ctclm::NgSlot *slots, unsigned n) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ng[idx[i]] = slots[i];
}
static int cb_sync(ctcd_scorer *s, hipStream_t stream = nullptr) {
  ctclm::CallbackLm &c = *s->cbl;
  ctclm::HostScorer &h = c.hs;
  if (c.rehashed || s->cb_ng_slots != h.ng.size()) {
    if (s->cb_ng_slots != h.ng.size()) {
      if (s->cb_ng) (void)hipFree(s->cb_ng);
      s->cb_ng = nullptr;
      HIP_TRY(hipMalloc((void **)&s->cb_ng, h.ng.size() * sizeof(ctclm::NgSlot)));
      s->cb_ng_slots = h.ng.size();
    }
    HIP_TRY(hipMemcpy(s->cb_ng, h.ng.data(), h.ng.size() * sizeof(ctclm::NgSlot), hipMemcpyHostToDevice));
  } else if (!c.dirty.empty()) {
    // (round 5) the slots written since the last launch travel in ONE copy -- [their indices | the slots] -- and a kernel puts
    // them in place.  (Rounds 1-4: one blocking 16-byte hipMemcpy per slot -- ~10 us each, 500 a round at the configs[4] shape:
    // two thirds of a round's 8 ms.)
    const size_t n = c.dirty.size();
    if (s->cb_stage_cap < n) {  // (both ends of the copy grow together; the host end is page-locked: the copy is queued on `stream`, in front
                                //  of the scatter kernel, and its ordering comes from the stream -- ADVICE r5)
      if (stream) HIP_TRY(hipStreamSynchronize(stream)); else HIP_TRY(hipDeviceSynchronize());
      if (s->cb_stage) (void)hipFree(s->cb_stage);
      if (s->cb_stage_hp) (void)hipHostFree(s->cb_stage_hp);
      s->cb_stage = nullptr; s->cb_stage_hp = nullptr; s->cb_stage_cap = 0;
      const size_t cap = n * 2 + 1024;
      HIP_TRY(hipMalloc((void **)&s->cb_stage, cap * (4 + sizeof(ctclm::NgSlot))));
      HIP_TRY(hipHostMalloc((void **)&s->cb_stage_hp, cap * (4 + sizeof(ctclm::NgSlot)), hipHostMallocDefault));
      s->cb_stage_cap = cap;
    }
    if (!s->cb_stage_ev) HIP_TRY(hipEventCreateWithFlags(&s->cb_stage_ev, hipEventDisableTiming));
    HIP_TRY(hipEventSynchronize(s->cb_stage_ev));  // (the previous copy out of this block -- possibly queued by a call that has returned)
    uint32_t *hi = (uint32_t *)s->cb_stage_hp;
    ctclm::NgSlot *hsl = (ctclm::NgSlot *)(s->cb_stage_hp + n * 4);
    for (size_t k = 0; k < n; ++k) { hi[k] = c.dirty[k]; hsl[k] = h.ng[c.dirty[k]]; }
    HIP_TRY(hipMemcpyAsync(s->cb_stage, s->cb_stage_hp, n * (4 + sizeof(ctclm::NgSlot)), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(s->cb_stage_ev, stream));
    hipLaunchKernelGGL(cb_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (ctclm::NgSlot *)s->cb_ng, (const uint32_t *)s->cb_stage,
                       (const ctclm::NgSlot *)(s->cb_stage + n * 4), (unsigned)n);
    HIP_TRY(hipGetLastError());
  }
  c.rehashed = false;
  c.dirty.clear();
  if (s->cb_st_cap < h.st_bo.size()) {  // every state backs off to the empty context with weight 0: two zeroed arrays
    if (s->cb_st) (void)hipFree(s->cb_st);
    s->cb_st = nullptr;
    const size_t cap = std::max<size_t>(h.st_bo.size() * 2, s->h_live ? kCbLiveStates0 : (size_t)1 << 20);  // (head room: a waiting launch cannot have them replaced)
    HIP_TRY(hipMalloc((void **)&s->cb_st, cap * 8));
    HIP_TRY(hipMemset(s->cb_st, 0, cap * 8));
    s->cb_st_cap = cap;
  }
  s->dview.ng = (const ctclm::NgSlot *)s->cb_ng;
  s->dview.ng_mask = (uint32_t)h.ng.size() - 1;
  s->dview.st_bo = (const float *)s->cb_st;
  s->dview.st_fail = (const uint32_t *)(s->cb_st + s->cb_st_cap * 4);
  return CTCD_OK;
}

static int create_callback_scorer(ctcd_scorer **out, double alpha, double beta, int max_order, const char *const *vocabulary, int n_vocabulary,
                                  ctclm::CondLog10Fn fn, ctclm::CondLog10BatchFn bfn, void *user, const char *const *labels, int V, int device_id) {
  if (!out || (!fn && !bfn) || !labels || V <= 0 || n_vocabulary < 0 || (n_vocabulary && !vocabulary)) return fail(CTCD_EINVAL, "bad scorer arguments");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev) return fail(CTCD_EINVAL, "no such HIP device");
  std::vector<std::string> lab(V), voc(n_vocabulary);
  for (int i = 0; i < V; ++i) { if (!labels[i]) return fail(CTCD_EINVAL, "null label"); lab[i] = labels[i]; }
  for (int i = 0; i < n_vocabulary; ++i) { if (!vocabulary[i]) return fail(CTCD_EINVAL, "null vocabulary word"); voc[i] = vocabulary[i]; }
  ctcd_scorer *s = new ctcd_scorer;
  s->device = device_id;
  s->cbl = new ctclm::CallbackLm;
  s->ask_pool.cl = s->cbl;
  if (!s->cbl->build(alpha, beta, max_order, voc, lab, fn, user, bfn)) {
    const std::string msg = s->cbl->hs.error;
    ctcd_scorer_destroy(s);
    return fail(CTCD_EINVAL, msg);
  }
  const ctclm::HostScorer &h = s->cbl->hs;
  // the scalar facts the accessors and the launches read (the tables stay with the callback object)
  s->host.alpha = alpha; s->host.beta = beta; s->host.order = h.order; s->host.char_based = h.char_based; s->host.dict_size = h.dict_size;
  s->host.space_id = h.space_id; s->host.labels = h.labels; s->host.dict_wide = h.dict_wide;
  CTC_ON_DEVICE(device_id);
  size_t off = 0;
  auto place = [&off](size_t bytes) { const size_t o = off; off = (off + bytes + 255) / 256 * 256; return o; };
  const size_t o_up = place(h.uni_prob.size() * 4), o_us = place(h.uni_state.size() * 4), o_dc = place(h.dict.size() * sizeof(ctclm::DictNode)),
               o_lw = place(h.label_word.size() * 4), o_dl = place(h.dict_lab.size() * 4);
  hipError_t e = hipMalloc((void **)&s->cb_uni, off ? off : 256);
  if (e == hipSuccess) e = hipMalloc((void **)&s->cb_miss, (size_t)kCbMissCap * sizeof(ctclm::MissEntry) + 256);
  if (e != hipSuccess) { ctcd_scorer_destroy(s); return fail(CTCD_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  auto up = [&](size_t o, const void *src, size_t bytes) { return bytes ? hipMemcpy(s->cb_uni + o, src, bytes, hipMemcpyHostToDevice) : hipSuccess; };
  if ((e = up(o_up, h.uni_prob.data(), h.uni_prob.size() * 4)) != hipSuccess || (e = up(o_us, h.uni_state.data(), h.uni_state.size() * 4)) != hipSuccess ||
      (e = up(o_dc, h.dict.data(), h.dict.size() * sizeof(ctclm::DictNode))) != hipSuccess ||
      (e = up(o_lw, h.label_word.data(), h.label_word.size() * 4)) != hipSuccess || (e = up(o_dl, h.dict_lab.data(), h.dict_lab.size() * 4)) != hipSuccess) {
    ctcd_scorer_destroy(s);
    return fail(CTCD_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  s->dview = h.view();
  s->dview.uni_prob = (const float *)(s->cb_uni + o_up); s->dview.uni_state = (const uint32_t *)(s->cb_uni + o_us);
  s->dview.dict = (const ctclm::DictNode *)(s->cb_uni + o_dc); s->dview.label_word = (const uint32_t *)(s->cb_uni + o_lw);
  s->dview.dict_lab = (const uint32_t *)(s->cb_uni + o_dl);
  s->dview.cb = 1;
  s->dview.cb_count = (unsigned *)s->cb_miss;
  s->dview.cb_miss = (ctclm::MissEntry *)(s->cb_miss + 256);
  s->dview.cb_cap = kCbMissCap;
  // the miss list itself lives in page-locked memory the host reads while a launch runs (the counter stays on the device)
  if (hipHostMalloc((void **)&s->h_live, kLiveBytes, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
      hipHostGetDevicePointer((void **)&s->d_live, s->h_live, 0) == hipSuccess) {
    std::memset(s->h_live, 0, kLiveOffMiss);
    std::memset(s->h_live + kLiveOffMiss, 0xff, (size_t)kCbMissCap * sizeof(ctclm::MissEntry));
    s->dview.cb_miss = (ctclm::MissEntry *)(s->d_live + kLiveOffMiss);
  } else {
    if (s->h_live) (void)hipHostFree(s->h_live);
    s->h_live = nullptr; s->d_live = nullptr;
    (void)hipGetLastError();
  }
  if (s->h_live) {  // (a waiting launch cannot have its tables moved: they get their room here, not in the first decode)
    s->cbl->grow(kCbLiveSlots0);
    s->live_stamp.assign(s->cbl->hs.ng.size(), 0u);
  }
  const int rc = cb_sync(s);
  if (rc) { ctcd_scorer_destroy(s); return rc; }
  *out = s;
  return CTCD_OK;
}
int ctcd_scorer_create_callback(ctcd_scorer **out, double alpha, double beta, int max_order, const char *const *vocabulary, int n_vocabulary,
                                ctcd_cond_log10_fn fn, void *user, const char *const *labels, int V, int device_id) {
  if (!fn) return fail(CTCD_EINVAL, "bad scorer arguments");
  return create_callback_scorer(out, alpha, beta, max_order, vocabulary, n_vocabulary, (ctclm::CondLog10Fn)fn, nullptr, user, labels, V, device_id);
}
int ctcd_scorer_create_callback_batch(ctcd_scorer **out, double alpha, double beta, int max_order, const char *const *vocabulary, int n_vocabulary,
                                      ctcd_cond_log10_batch_fn fn, void *user, const char *const *labels, int V, int device_id) {
  if (!fn) return fail(CTCD_EINVAL, "bad scorer arguments");
  return create_callback_scorer(out, alpha, beta, max_order, vocabulary, n_vocabulary, nullptr, (ctclm::CondLog10BatchFn)fn, user, labels, V, device_id);
}
int ctcd_scorer_is_character_based(const ctcd_scorer *s) { return s ? (s->host.char_based ? 1 : 0) : -1; }
int ctcd_scorer_max_order(const ctcd_scorer *s) { return s ? s->host.order : -1; }
int ctcd_scorer_dict_size(const ctcd_scorer *s) { return s ? s->host.dict_size : -1; }
int ctcd_scorer_reset_params(ctcd_scorer *s, double alpha, double beta) {
  if (!s) return fail(CTCD_EINVAL, "scorer == NULL");
  s->host.alpha = alpha;
  s->host.beta = beta;
  return CTCD_OK;
}
double ctcd_scorer_cond_log_prob(const ctcd_scorer *s, const char *const *words, int n) {
  if (!s || !words || n < 0) return 0.0;
  if (s->cbl) {  // the callback itself, with the reference's conversion (scorer.cpp:74-93)
    float p10 = 0.f;
    const int rc = n > 0 ? s->cbl->ask_one(words, n, &p10) : 1;
    return rc == 0 ? (double)p10 / (double)0.4342944819f : ctclm::kOovScore;
  }
  std::vector<std::string> w(n);
  for (int i = 0; i < n; ++i) w[i] = words[i] ? words[i] : "";
  return s->host.cond_log_prob(w);
}
// ... and in the form the scorer hook speaks (ctcd_cond_log10_fn): the float32 log10 probability before the reference's
// conversion; returns 1 for a window with an unknown word.  Lets the built-in tables serve as a callback (tests, adapters).
int ctcd_scorer_cond_log10(const ctcd_scorer *s, const char *const *words, int n, float *log10_prob) {
  if (!s || !words || n <= 0 || !log10_prob) return -1;
  if (s->cbl) return s->cbl->ask_one(words, n, log10_prob);
  // (HostScorer::cond_log10 without the vector of strings: this function is what bench.py puts behind the hook as a native callback)
  const ctclm::LmView v = s->host.view();
  uint32_t st = 0;
  float p = 0.f;
  std::string key;
  for (int i = 0; i < n; ++i) {
    key.assign(words[i] ? words[i] : "");
    const uint32_t id = s->host.id_of(key);
    if (id == 0) return 1;
    p = ctclm::lm_score(v, st, id, &st);
  }
  *log10_prob = p;
  return 0;
}
// ... and the batched form (ctcd_cond_log10_batch_fn): window after window through ctcd_scorer_cond_log10
int ctcd_scorer_cond_log10_batch(const ctcd_scorer *s, const char *const *words, int n_windows, int order, float *log10_probs, int32_t *status) {
  if (!s || !words || n_windows < 0 || order <= 0 || (n_windows && (!log10_probs || !status))) return -1;
  for (int i = 0; i < n_windows; ++i) {
    float p = 0.f;
    const int rc = ctcd_scorer_cond_log10(s, words + (size_t)i * order, order, &p);
    if (rc < 0) return rc;
    log10_probs[i] = rc == 0 ? p : 0.f;
    status[i] = rc;
  }
  return 0;
}
int ctcd_scorer_set_callback_threads(ctcd_scorer *s, int threads) {
  if (!s || !s->cbl) return fail(CTCD_EINVAL, "not a callback scorer");
  if (threads < 1 || threads > 64) return fail(CTCD_EINVAL, "callback threads must be in [1, 64]");
  if (s->cbl->bfn && threads != 1) return fail(CTCD_EUNSUPPORTED, "a batched callback is called from the decoding thread only (no helper threads)");
  std::lock_guard<std::mutex> lk(s->cb_mu);
  s->ask_pool.start(threads, s->cbl);
  return CTCD_OK;
}
long long ctcd_scorer_callback_calls(const ctcd_scorer *s) { return s && s->cbl ? (long long)s->cbl->queries : 0; }
double ctcd_scorer_callback_seconds(const ctcd_scorer *s) { return s && s->cbl ? s->cbl->cb_seconds : 0.0; }
long long ctcd_scorer_callback_batches(const ctcd_scorer *s) { return s && s->cbl ? (long long)s->cbl->batches : 0; }

// Decoding with a callback scorer (ctcd_scorer_create_callback).  A launch decodes until an utterance asks for a (history, word)
// pair the device cache does not hold, parks that utterance in front of the frame it was in (every utterance runs as a stream:
// the caller's own, or a temporary one) and queues the pair; the host asks the callback, inserts the answers and launches
// again -- the parked utterances resume where they stopped, the finished ones pass through untouched -- until every utterance
// has consumed its rows.  Results equal those of a scorer whose tables were complete from the start (tests: the built-in ARPA
// tables behind the callback, bit for bit).  A capability, not a fast path: a launch per round of misses plus the callback's
// own time; a warm cache needs one launch.
static int cb_rounds(ctcd_decoder *d, ctcd_stream **states, const unsigned char *is_eos, const int32_t *lens, const float *probs, int B, int T, int V,
                     int beam, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input, ctcd_scorer *scorer, int32_t *out_tok,
                     int32_t *out_ts, float *out_sc, int32_t *out_len, int32_t *n_results, int out_T, void *stream_, const CompactOut *co = nullptr,
                     bool one_shot = false, int in_dtype = -1) {
  // (the callback runs under this lock: a callback that decodes with the same scorer deadlocks -- include/ctcdecode_amd.h)
  std::lock_guard<std::mutex> cache_lock(scorer->cb_mu);
  hipStream_t stream = (hipStream_t)stream_;
  int rc0;
  if ((rc0 = d->cb_ctl.ensure((size_t)B * 12 + 256))) return rc0;  // [frame offsets | frames done | row lengths] (kept: no hipMalloc / hipFree per call)
  int *d_off = (int *)d->cb_ctl.p, *d_done = d_off + B, *d_rows = d_done + B;
  if (d->h_cb_items < (size_t)B) {
    if (d->h_cb) (void)hipHostFree(d->h_cb);
    d->h_cb = nullptr;
    HIP_TRY(hipHostMalloc((void **)&d->h_cb, ((size_t)B * 2 + 4) * 4, hipHostMallocDefault));
    d->h_cb_items = (size_t)B;
  }
  int32_t *st_h = d->h_cb, *fd_h = d->h_cb + B;
  unsigned *nmiss_h = (unsigned *)(d->h_cb + 2 * (size_t)B);
  HIP_TRY(hipMemcpyAsync(d_rows, lens, (size_t)B * 4, hipMemcpyHostToDevice, stream));
  std::vector<int32_t> done(B, 0), rem(B);
  std::vector<unsigned char> eos(B), finished(B, 0);
  std::vector<uint32_t> miss;
  int rc;
  // The launch that waits (decode_kernel.h KernelArgs::cb_log_len): a workgroup whose utterance misses stays on its CU while this
  // thread -- polling the miss list in page-locked memory -- asks the callback and publishes the answered slots; a round of misses
  // costs two PCIe crossings instead of a launch.  What it cannot do while the kernel runs -- move the table (rehash), lengthen the
  // state arrays, hold more than its log -- ends the wait: the workgroups leave as they always did and the loop below relaunches.
  static const bool live_off = getenv("CTCD_HOOK_WAIT") && atoi(getenv("CTCD_HOOK_WAIT")) == 0;
  const bool live = scorer->h_live && !live_off && !d->no_hook_wait && (uint32_t)B <= kCbLiveItems;
  ctclm::CallbackLm &cl = *scorer->cbl;
  d->last_cb_waits = 0;
  // ctcd_last_scorer_pairs: every queued pair the host reads is counted; a pair counts as a repeat of the same item when the item that
  // queued it first in this decode queues it again (per cache slot: the stamps restart when the table moves)
  const unsigned long long asked0 = cl.queries;
  long long n_queued = 0, n_same = 0;
  const uint32_t call_id = ++scorer->pair_call;
  d->last_pairs[0] = d->last_pairs[1] = d->last_pairs[2] = 0;
  auto note_pair = [&](uint32_t at, uint32_t item) {
    ++n_queued;
    if (scorer->pair_seen.size() != cl.hs.ng.size()) scorer->pair_seen.assign(cl.hs.ng.size(), 0ull);
    if (at >= scorer->pair_seen.size()) return;
    uint64_t &e = scorer->pair_seen[at];
    if ((uint32_t)(e >> 32) == call_id) n_same += (uint32_t)e == item;
    else e = ((uint64_t)call_id << 32) | item;
  };
  const bool filter_off = d->no_lmq_filter;
  for (int round = 0;; ++round) {
    d->last_cb_rounds = round;
    if (round > 4 * T + 64) return fail(CTCD_EINTERNAL, "scorer hook: the decode does not make progress");
    if (live) {  // head room for the answers of a waiting launch: 8192 more slots / states before anything has to move
      if ((cl.used + 8192) * 2 > cl.hs.ng.size()) cl.grow(std::max<size_t>(cl.hs.ng.size() * 4, kCbLiveSlots0));  // (64 MB to begin with)
      if (cl.n_states() + 8192 >= scorer->cb_st_cap / 2 && cl.hs.st_bo.size() <= scorer->cb_st_cap) {  // (cb_sync doubles the device arrays)
        cl.hs.st_bo.resize(scorer->cb_st_cap + 64, 0.0f);
        cl.hs.st_fail.resize(cl.hs.st_bo.size(), 0u);
      }
    }
    if ((rc = cb_sync(scorer, stream))) return rc;
    int left = 0;
    bool any_eos = false;
    for (int b = 0; b < B; ++b) {
      rem[b] = finished[b] ? 0 : lens[b] - done[b];
      eos[b] = finished[b] ? 0 : is_eos[b];
      any_eos |= eos[b] != 0;
      left += !finished[b];
    }
    if (!left) break;
    HIP_TRY(hipMemcpyAsync(d_off, done.data(), (size_t)B * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(scorer->cb_miss, 0, 4, stream));
    scorer->dview.cb = filter_off ? 2 : 1;  // (beam_core.h lm_cond_: 2 = queue every miss, without the per-utterance filter)
    StreamCall sc{states, eos.data(), out_T, rem.data(), any_eos};
    sc.no_clear = round > 0;
    sc.frame_off = d_off;
    sc.frames_done = d_done;
    sc.row_lens = d_rows;
    sc.one_shot = one_shot;
    sc.in_dtype = in_dtype;
    volatile unsigned *h_len = (volatile unsigned *)scorer->h_live;
    volatile int32_t *h_done = (volatile int32_t *)(scorer->h_live + kLiveOffDone);
    volatile uint32_t *h_miss = (volatile uint32_t *)(scorer->h_live + kLiveOffMiss);  // (four words per pair: ctclm::MissEntry)
    volatile unsigned *h_ans = (volatile unsigned *)(scorer->h_live + kLiveOffAns);
    if (scorer->h_live) {  // (the miss list of the last launch: back to "not written")
      std::memset(scorer->h_live + kLiveOffMiss, 0xff, (size_t)scorer->live_miss_hw * sizeof(ctclm::MissEntry));
      scorer->live_miss_hw = 0;
    }
    if (live) {
      *h_len = 0;
      for (int b = 0; b < B; ++b) { h_done[b] = finished[b] ? 1 : 0; h_ans[b] = 0; }
      std::atomic_thread_fence(std::memory_order_seq_cst);
      sc.live = scorer->d_live;
    }
    if ((rc = decode_common(d, probs, nullptr, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, out_tok, out_ts, out_sc, out_len,
                            n_results, stream_, &sc, scorer, co)))
      return rc;
    // (one page-locked block: the three reports arrive behind the launch without staging copies)
    HIP_TRY(hipMemcpyAsync(st_h, d->status.p, (size_t)B * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(fd_h, d_done, (size_t)B * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(nmiss_h, scorer->cb_miss, 4, hipMemcpyDeviceToHost, stream));
    unsigned long long seen = 0;  // miss-list entries answered while the launch ran (the list is a ring then: entry i sits at i mod capacity)
    if (live) {
      uint32_t *l_idx = (uint32_t *)(scorer->h_live + kLiveOffIdx);
      ctclm::NgSlot *l_slot = (ctclm::NgSlot *)(scorer->h_live + kLiveOffSlot);
      // a slot goes into the log once per launch: a workgroup that asks for a pair the log already holds finds it there (it applies
      // the log before it waits), so the duplicates -- every park queues what its pending entries need -- cost a table probe each
      if (scorer->live_stamp.size() != cl.hs.ng.size()) scorer->live_stamp.assign(cl.hs.ng.size(), 0u);
      const uint32_t launch_id = ++scorer->live_launch;
      scorer->live_memo.assign((size_t)1 << 16, 0ull);
      scorer->live_memo_at.assign((size_t)1 << 16, 0u);
      if (scorer->pair_seen.size() != cl.hs.ng.size()) scorer->pair_seen.assign(cl.hs.ng.size(), 0ull);
      unsigned log_n = 0;
      bool give_up = false;
      std::vector<unsigned> ans_local((size_t)B, 0u);
      auto t_last = std::chrono::steady_clock::now();
      static const bool trace = getenv("CTCD_HOOK_TIMING") != nullptr;  // (stderr: how busy this thread is while a launch waits on it)
      const auto t_begin = t_last;
      double busy = 0.0;
      scorer->ask_pool.begin();
      for (unsigned spin = 0;; ++spin) {
        const unsigned long long s0 = seen;
        const auto t_in = trace ? std::chrono::steady_clock::now() : t_begin;
        unsigned fresh = 0;
        for (bool more = true; more && !give_up;) {
          // The pairs that have arrived, up to 128 at a time, in three passes.  (1) classify: answered moments ago (memo), cached, or new to
          // the cache -- the table lines were requested while the pairs were read (a cold probe of a table of tens of MB is a DRAM access),
          // the words of a new window are looked up and the line of its next state requested; (2) ask the callback about the new windows
          // (the scorer's helper threads take a share each when it has any); (3) in the order of the list: cache the answers, append to
          // the log, publish per item.
          // (a batched callback: up to ctclm::kBatchWindows pairs per pass, their new windows in one call)
          enum { kMemo = 0, kHave = 1, kNew = 2, kDup = 3 };
          constexpr int kBatch = 128, kBatchMax = ctclm::kBatchWindows > kBatch ? ctclm::kBatchWindows : kBatch;
          const int batch = cl.bfn ? kBatchMax : kBatch;
          struct Pend { uint32_t st, wd, item, at; size_t ring; int kind; } pend[kBatchMax];
          ctclm::CallbackLm::Ask asks[kBatchMax];
          int np = 0, na = 0;
          const uint32_t mask = (uint32_t)cl.hs.ng.size() - 1;
          while (np < batch) {
            const size_t at_ring = (size_t)((seen + (unsigned)np) & (kCbMissCap - 1));
            if (h_miss[4 * at_ring + 3] == 0xFFFFFFFFu) { more = false; break; }  // (the flag word: the pair's 16 bytes arrive in one piece)
            std::atomic_thread_fence(std::memory_order_acquire);
            pend[np] = Pend{h_miss[4 * at_ring], h_miss[4 * at_ring + 1], h_miss[4 * at_ring + 2], 0u, at_ring, kMemo};
            const uint32_t hh = ctclm::ng_hash(pend[np].st, pend[np].wd) & mask;
            __builtin_prefetch(&cl.hs.ng[hh]);
            __builtin_prefetch(&scorer->live_stamp[hh]);
            __builtin_prefetch(&scorer->pair_seen[hh]);
            ++np;
          }
          bool bad = false;
          int usable = np;  // (the table runs out of room at this pair: the ones before it are served, then the wait ends)
          for (int q = 0; q < np; ++q) {
            Pend &e = pend[q];
            // most of the list repeats pairs asked moments ago (every park queues what its pending entries need, neighbouring prefixes
            // and utterances want the same windows): a small direct-mapped memo of the pairs already in this launch's log answers
            // those without touching the table
            const unsigned long long key = ((unsigned long long)e.st << 32) | e.wd;
            const size_t mi = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 48);
            if (scorer->live_memo[mi] == key) { e.at = scorer->live_memo_at[mi]; continue; }  // kMemo
            const long long have = cl.find_slot(e.st, e.wd);
            if (have >= 0) { e.kind = kHave; e.at = (uint32_t)have; continue; }
            e.kind = kNew;
            for (int o = 0; o < q; ++o)  // (the same new pair twice in one batch: the callback is asked once per window)
              if (pend[o].kind == kNew && pend[o].st == e.st && pend[o].wd == e.wd) { e.kind = kDup; break; }
            if (e.kind == kDup) continue;
            if (!cl.room_for((size_t)na + 1, scorer->cb_st_cap)) { usable = q; give_up = true; break; }  // (the tables would have to move: between launches)
            if (!cl.prepare(e.st, e.wd, asks[na])) { bad = true; break; }
            cl.prefetch_next_state(e.st, e.wd);
            ++na;
          }
          if (!bad && na) {
            const auto t0 = std::chrono::steady_clock::now();
            if (cl.bfn) cl.ask_many(asks, na);
            else scorer->ask_pool.ask_all(asks, na);
            cl.cb_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
          }
          int ia = 0;
          bool log_full = false;
          for (int q = 0; q < usable && !bad; ++q) {
            Pend &e = pend[q];
            const size_t at_ring = e.ring;
            if (log_full && e.kind == kMemo) continue;
            const unsigned long long key = ((unsigned long long)e.st << 32) | e.wd;
            if (e.kind == kMemo) note_pair(e.at, e.item);
            if (e.kind != kMemo) {
              uint32_t at = e.at;
              if (e.kind == kNew) {
                if (!cl.commit(asks[ia++], &at)) { bad = true; break; }
              } else if (e.kind == kDup) {
                at = (uint32_t)cl.find_slot(e.st, e.wd);
              }
              if (log_full) continue;  // (the answers that have been paid for are cached; their pairs stay on the list for the next launch)
              note_pair(at, e.item);
              if (scorer->live_stamp[at] != launch_id) {
                if (log_n >= kCbLogCap) { give_up = true; log_full = true; continue; }
                scorer->live_stamp[at] = launch_id;
                l_idx[log_n] = at;
                l_slot[log_n] = cl.hs.ng[at];
                ++log_n;
                ++fresh;
                std::atomic_thread_fence(std::memory_order_release);
                *h_len = log_n;  // (published entry by entry: the stores of this thread arrive in order)
              }
              const size_t mi = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 48);
              scorer->live_memo[mi] = key;  // (in the log from here on)
              scorer->live_memo_at[mi] = at;
            }
            if (e.item < (uint32_t)B) {  // the item's workgroup goes on when every pair it queued has been dealt with
              std::atomic_thread_fence(std::memory_order_release);
              h_ans[e.item] = ++ans_local[e.item];
            }
            h_miss[4 * at_ring] = 0xFFFFFFFFu; h_miss[4 * at_ring + 1] = 0xFFFFFFFFu; h_miss[4 * at_ring + 2] = 0xFFFFFFFFu; h_miss[4 * at_ring + 3] = 0xFFFFFFFFu;
            ++seen;
          }
          if (bad) {
            scorer->ask_pool.end();
            *h_len = 0xFFFFFFFFu;
            (void)hipStreamSynchronize(stream);
            scorer->live_miss_hw = kCbMissCap;
            return fail(CTCD_EINVAL, cl.hs.error);
          }
        }
        if (fresh) ++d->last_cb_waits;
        if (seen > s0) {
          t_last = std::chrono::steady_clock::now();
          if (trace) busy += std::chrono::duration<double>(t_last - t_in).count();
        }
        bool all = true;
        for (int b = 0; b < B && all; ++b) all = h_done[b] != 0;
        if (all) break;
        if (!give_up && (spin & 1023) == 1023) {
          // (nothing new for a second with workgroups still out, or a launch that has ended some other way)
          if (std::chrono::steady_clock::now() - t_last > std::chrono::seconds(1) || hipStreamQuery(stream) != hipErrorNotReady) give_up = true;
          (void)hipGetLastError();
        }
        if (give_up) { *h_len = 0xFFFFFFFFu; break; }
        __builtin_ia32_pause();
      }
      scorer->ask_pool.end();
      if (trace) fprintf(stderr, "scorer hook, waiting launch %d: %.2f ms, this thread busy %.2f ms with %llu queued pairs (%u new to the launch's log)%s\n", round,
                         1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(), 1e3 * busy, seen, log_n, give_up ? "; gave up" : "");
    }
    HIP_TRY(hipStreamSynchronize(stream));
    const unsigned nmiss = *nmiss_h;
    scorer->live_miss_hw = live ? kCbMissCap : (nmiss < kCbMissCap ? nmiss : kCbMissCap);  // (a ring may hold unconsumed pairs anywhere)
    bool need = false;
    for (int b = 0; b < B; ++b) {
      if (finished[b]) continue;
      if (st_h[b] == ST_OK) { finished[b] = 1; continue; }
      if (st_h[b] == ST_CB_DANGER)
        return fail(CTCD_EUNSUPPORTED, "a callback scorer does not support rows with infinite / overflowing log-probabilities (item " + std::to_string(b) + ")");
      if (st_h[b] != ST_NEED_HOST) return fail(CTCD_EINTERNAL, "decoder status " + std::to_string(st_h[b]) + " for item " + std::to_string(b));
      done[b] = (int32_t)(fd_h[b] - states[b]->frames);  // (the parked state counts the stream's frames; the rows, this call's)
      need = true;
    }
    if (need) {
      if (nmiss == 0) return fail(CTCD_EINTERNAL, "scorer hook: an utterance waits for the host but queued nothing");
      if (live) {  // what the ring still holds (the launch has ended: every pair queued is written)
        miss.clear();
        for (size_t i = 0; i < (size_t)kCbMissCap; ++i)
          if (h_miss[4 * i + 3] != 0xFFFFFFFFu) miss.insert(miss.end(), {h_miss[4 * i], h_miss[4 * i + 1], h_miss[4 * i + 2], h_miss[4 * i + 3]});
        const size_t take = miss.size() / 4;
        std::vector<uint32_t> at(take);
        if (!cl.resolve_many(miss.data(), take, 4, at.data())) return fail(CTCD_EINVAL, cl.hs.error);
        for (size_t i = 0; i < take; ++i) note_pair(at[i], miss[4 * i + 2]);
      } else {
        const unsigned take = nmiss < kCbMissCap ? nmiss : kCbMissCap;  // (pairs beyond the list's capacity are asked for again next round)
        miss.resize((size_t)4 * take);
        if (scorer->h_live) {  // (the list is in page-locked memory)
          for (size_t i = 0; i < (size_t)4 * take; ++i) miss[i] = h_miss[i];
        } else {
          HIP_TRY(hipMemcpy(miss.data(), scorer->cb_miss + 256, (size_t)take * sizeof(ctclm::MissEntry), hipMemcpyDeviceToHost));
        }
        std::vector<uint32_t> at(take);
        if (!cl.resolve_many(miss.data(), take, 4, at.data())) return fail(CTCD_EINVAL, cl.hs.error);
        for (unsigned i = 0; i < take; ++i) note_pair(at[i], miss[4 * i + 2]);
      }
    }
  }
  d->last_pairs[0] = n_queued;
  d->last_pairs[1] = (long long)(cl.queries - asked0);
  d->last_pairs[2] = n_same;
  return CTCD_OK;
}

// ... for a whole batch: temporary streams in one allocation, a block per utterance sized for all T frames
static int decode_lm_callback(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam, double cutoff_prob,
                              int cutoff_top_n, int blank_id, int log_input, ctcd_scorer *scorer, int32_t *out_tok, int32_t *out_ts,
                              float *out_sc, int32_t *out_len, int32_t *n_results, void *stream_, const CompactOut *co = nullptr) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  if (B <= 0 || T < 0 || beam <= 0 || beam > kMaxBeam) return B == 0 ? CTCD_OK : fail(CTCD_EINVAL, "bad arguments");
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<int32_t> len(B, T);
  if (seq_lens) {
    HIP_TRY(hipMemcpyAsync(len.data(), seq_lens, (size_t)B * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int b = 0; b < B; ++b) len[b] = len[b] < 0 ? 0 : (len[b] > T ? T : len[b]);  // binding.cpp:64-65
  }
  const long long capf = T > 0 ? T : 1;
  const size_t blk = (stream_block_bytes(capf, beam) + 255) / 256 * 256;
  // (round 5: the blocks stay with the decoder -- rounds 1-4 allocated and freed them in every call, 384 MB at the configs[4]
  //  shape, and zeroed them with two memsets per utterance: a warm cache cost three times the built-in tables' decode)
  int rcb;
  if ((rcb = d->cb_blocks.ensure(blk * (size_t)B))) return rcb;
  char *blocks = (char *)d->cb_blocks.p;
  std::vector<ctcd_stream> sts(B);
  std::vector<ctcd_stream *> states(B);
  for (int b = 0; b < B; ++b) {
    ctcd_stream &st = sts[b];
    st.device = d->device; st.scorer = scorer; st.block = blocks + (size_t)b * blk; st.bytes = blk; st.V = V; st.beam = beam; st.frames = 0; st.cap_frames = capf;
    states[b] = &st;
  }
  // frames == 0: the first launch initialises the beam; the high parts of the nodes' time steps start at zero
  HIP_TRY(hipMemset2DAsync(blocks, blk, 0, stream_pool_offset(beam), (size_t)B, stream));
  HIP_TRY(hipMemset2DAsync(blocks + stream_thi_offset(capf, beam), blk, 0, stream_nodes(capf, beam) * sizeof(int), (size_t)B, stream));
  const std::vector<unsigned char> eos(B, 1);
  return cb_rounds(d, states.data(), eos.data(), len.data(), probs, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, scorer, out_tok,
                   out_ts, out_sc, out_len, n_results, T, stream_, co, true);
}

int ctcd_beam_decode_lm(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                        int /*num_processes*/, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input, ctcd_scorer *scorer,
                        int32_t *out_tok, int32_t *out_ts, float *out_sc, int32_t *out_len, int32_t *n_results, void *stream_) {
  if (!scorer) return fail(CTCD_EINVAL, "scorer == NULL (use ctcd_beam_decode)");
  if (scorer->cbl)
    return decode_lm_callback(d, probs, seq_lens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, scorer, out_tok, out_ts, out_sc,
                              out_len, n_results, stream_);
  return decode_common(d, probs, seq_lens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, out_tok, out_ts, out_sc,
                       out_len, n_results, stream_, nullptr, scorer);
}

// ---- streaming: DecoderState kept between calls (ctcdecode/__init__.py:143-272, binding.cpp:153-265)
int ctcd_stream_create_lm(ctcd_decoder *d, ctcd_stream **out, int V, int beam, int frames_hint, ctcd_scorer *scorer) {
  int rc = ctcd_stream_create(d, out, V, beam, frames_hint);
  if (rc == CTCD_OK) (*out)->scorer = scorer;
  return rc;
}

int ctcd_stream_create(ctcd_decoder *d, ctcd_stream **out, int V, int beam, int frames_hint) {
  if (!d || !out || V <= 0 || beam <= 0 || beam > kMaxBeam) return fail(CTCD_EINVAL, "bad stream parameters");
  CTC_ON_DEVICE(d->device);
  ctcd_stream *st = new ctcd_stream;
  st->device = d->device;
  st->V = V;
  st->beam = beam;
  st->cap_frames = frames_hint > 0 ? frames_hint : 1024;
  st->hint_frames = st->cap_frames;
  st->bytes = stream_block_bytes(st->cap_frames, beam);
  hipError_t e = hipMalloc((void **)&st->block, st->bytes);
  if (e != hipSuccess) { delete st; return fail(CTCD_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  e = hipMemset(st->block, 0, stream_pool_offset(beam));  // frames == 0: the first call initialises the beam
  if (e == hipSuccess) e = hipMemset(st->block + stream_thi_offset(st->cap_frames, beam), 0, stream_nodes(st->cap_frames, beam) * sizeof(int));
  if (e != hipSuccess) { (void)hipFree(st->block); delete st; return fail(CTCD_EHIP, std::string("hipMemset: ") + hipGetErrorString(e)); }
  if (d->sk_on) {  // the blank-frame filter of live streams: the frame map is made with the stream, with room for the frames its pool takes
    st->map_cap = ctcsskip::map_grown_cap(0, st->cap_frames);
    e = hipMalloc((void **)&st->map, (size_t)st->map_cap * 4);
    if (e != hipSuccess) { (void)hipFree(st->block); delete st; return fail(CTCD_EHIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  }
  *out = st;
  return CTCD_OK;
}

void ctcd_stream_destroy(ctcd_decoder *d, ctcd_stream *st) {
  if (!st) return;
  DeviceGuard guard_(st->device);
  if (st->block) (void)hipFree(st->block);
  if (st->map) (void)hipFree(st->map);
  delete st;
}

long long ctcd_stream_frames(const ctcd_stream *st) { return st ? st->frames : -1; }

// ---- the blank-frame filter of live streams (stream_blank_skip.h) -------------------------------------------------------------------
int ctcd_set_stream_blank_skip(ctcd_decoder *d, int on, float cmp_prob, float cmp_log) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  if (on && (cmp_prob != cmp_prob || cmp_log != cmp_log)) return fail(CTCD_EINVAL, "ctcd_set_stream_blank_skip: the bounds are float32 numbers, not NaN");
  std::lock_guard<std::mutex> lock(d->mu_skip);
  d->sk_on = on != 0;
  d->sk_cmp_prob = cmp_prob;
  d->sk_cmp_log = cmp_log;
  return CTCD_OK;
}

long long ctcd_stream_frames_seen(const ctcd_stream *st) { return st ? (st->filtered ? st->seen : st->frames) : -1; }
long long ctcd_stream_map_bytes(const ctcd_stream *st) { return st ? st->map_cap * 4 : -1; }

int ctcd_last_stream_blank_skip(ctcd_decoder *d, long long *considered, long long *kept) {
  if (!d || !considered || !kept) return fail(CTCD_EINVAL, "ctcd_last_stream_blank_skip: null argument");
  std::lock_guard<std::mutex> lock(d->mu_skip);
  *considered = d->sk_last[0];
  *kept = d->sk_last[1];
  return CTCD_OK;
}

int ctcd_last_stream_blank_skip_ms(ctcd_decoder *d, float *filter_ms, float *wait_ms, float *remap_ms) {
  if (!d || !filter_ms || !wait_ms || !remap_ms) return fail(CTCD_EINVAL, "ctcd_last_stream_blank_skip_ms: null argument");
  std::lock_guard<std::mutex> lock(d->mu_skip);
  if (!d->ev_sk[0]) return fail(CTCD_EINVAL, "timing not enabled");
  CTC_ON_DEVICE(d->device);
  *filter_ms = *remap_ms = 0.f;
  *wait_ms = d->sk_wait_ms;
  if (d->sk_timed) {
    HIP_TRY(hipEventSynchronize(d->ev_sk[1]));
    HIP_TRY(hipEventElapsedTime(filter_ms, d->ev_sk[0], d->ev_sk[1]));
  }
  if (d->sk_remap_timed) {
    HIP_TRY(hipEventSynchronize(d->ev_sk[3]));
    HIP_TRY(hipEventElapsedTime(remap_ms, d->ev_sk[2], d->ev_sk[3]));
  }
  return CTCD_OK;
}

namespace {

// a stream adopts the filter at its first chunk: one that already has frames under the other setting is refused
int sskip_check_setting(const ctcd_decoder *d, ctcd_stream *const *states, int B, const char *who) {
  for (int b = 0; b < B; ++b) {
    const ctcd_stream *st = states[b];
    if (!st) return fail(CTCD_EINVAL, "stream state does not match the decoder configuration");
    if (d->sk_on ? (!st->filtered && st->frames > 0) : (st->filtered && st->seen > 0))
      return fail(CTCD_EINVAL, std::string(who) + ": item " + std::to_string(b) +
                                   (d->sk_on ? " has frames it took without the blank-frame filter this decoder has on"
                                             : " has frames it took through the blank-frame filter this decoder has off"));
  }
  return CTCD_OK;
}

// offsets of the arrays in the decoder's page-locked region: scan table | chunk lengths | kept counts | remap table.  Always taken for
// the region's capacity (d->h_sk_items), never for a call's batch: the remap table lies where no later call's scan arguments reach,
// whatever its batch size -- a remap kernel may still be reading it when the next chunk call fills in its own arguments.
struct SkRegion {
  size_t o_len, o_cnt, o_rtab, need;
  explicit SkRegion(size_t n) {
    o_len = n * sizeof(ctcsskip::StreamSkipItem);
    o_cnt = o_len + n * 4;
    o_rtab = (o_cnt + n * 4 + 15) & ~(size_t)15;
    need = o_rtab + n * sizeof(ctcsskip::StreamRemapItem);
  }
};

// (d->mu_skip held) the region with room for B items; a remap kernel that still reads the last table is waited for before it moves
int sskip_region(ctcd_decoder *d, int B, char **hb, char **db) {
  if (d->h_sk_items < (size_t)B) {
    if (d->sk_tab_busy) HIP_TRY(hipEventSynchronize(d->ev_sk_tab));
    d->sk_tab_busy = false;
    if (d->h_sk) (void)hipHostFree(d->h_sk);
    d->h_sk = nullptr;
    d->h_sk_items = 0;
    const size_t items = std::max<size_t>(2 * (size_t)B, 64);
    HIP_TRY(hipHostMalloc((void **)&d->h_sk, SkRegion(items).need, hipHostMallocMapped | hipHostMallocCoherent));
    d->h_sk_items = items;
  }
  if (!d->ev_sk_tab) HIP_TRY(hipEventCreateWithFlags(&d->ev_sk_tab, hipEventDisableTiming));
  *hb = d->h_sk;
  HIP_TRY(hipHostGetDevicePointer((void **)db, *hb, 0));
  return CTCD_OK;
}

// (d->mu_skip held) the remap table of a call, host and device address; the kernel that read the last one has finished
int sskip_remap_table(ctcd_decoder *d, int B, ctcsskip::StreamRemapItem **h_tab, const ctcsskip::StreamRemapItem **d_tab) {
  char *hb = nullptr, *db = nullptr;
  if (const int rc = sskip_region(d, B, &hb, &db)) return rc;
  if (d->sk_tab_busy) HIP_TRY(hipEventSynchronize(d->ev_sk_tab));
  d->sk_tab_busy = false;
  const SkRegion r(d->h_sk_items);
  *h_tab = (ctcsskip::StreamRemapItem *)(hb + r.o_rtab);
  *d_tab = (const ctcsskip::StreamRemapItem *)(db + r.o_rtab);
  return CTCD_OK;
}
int sskip_table_used(ctcd_decoder *d, hipStream_t stream) {
  HIP_TRY(hipEventRecord(d->ev_sk_tab, stream));
  d->sk_tab_busy = true;
  return CTCD_OK;
}
int sskip_timing_events(ctcd_decoder *d) {
  for (int i = 0; i < 4; ++i)
    if (!d->ev_sk[i]) HIP_TRY(hipEventCreate(&d->ev_sk[i]));
  return CTCD_OK;
}
// (d->mu_skip held) the row remap of a call's results, queued behind them: every stream's map and the frames it has decoded now
int sskip_remap_rows(ctcd_decoder *d, ctcd_stream **states, int B, int32_t *ts, const int32_t *lens, const int32_t *since, int rows_per_item,
                     long long row_stride, hipStream_t stream) {
  ctcsskip::StreamRemapItem *h_tab = nullptr;
  const ctcsskip::StreamRemapItem *d_tab = nullptr;
  if (const int rc = sskip_remap_table(d, B, &h_tab, &d_tab)) return rc;
  for (int b = 0; b < B; ++b) h_tab[b] = ctcsskip::StreamRemapItem{states[b]->map, nullptr, (int32_t)states[b]->frames, 0};
  d->sk_remap_timed = false;
  if (d->timing) {
    if (const int rc = sskip_timing_events(d)) return rc;
    HIP_TRY(hipEventRecord(d->ev_sk[2], stream));
  }
  const int e = ctcsskip::launch_remap_rows(ts, lens, since, d_tab, B, rows_per_item, row_stride, (void *)stream);
  if (e != (int)hipSuccess) return fail(CTCD_EHIP, std::string("ctc_stream_remap_rows_kernel: ") + hipGetErrorString((hipError_t)e));
  if (d->timing) {
    HIP_TRY(hipEventRecord(d->ev_sk[3], stream));
    d->sk_remap_timed = true;
  }
  return sskip_table_used(d, stream);
}

// what the filter hands a chunk call's decode: the kept rows, their counts as the chunk lengths, the log mode and element type to read them in
struct SkChunk {
  std::vector<int32_t> lens, kept;
  const float *rows = nullptr;
  int log_input = 0, dtype = CTCD_DTYPE_F32;
  long long considered = 0;
};

// (d->mu_skip held, the decoder's device current) The filter of one chunk call: every argument is checked before the device is touched;
// maps that lack room for the chunk grow; log-softmax (raw logits) -> scan -> gather are queued on `stream`, and the call waits for the
// B kept counts: stream_prepare sizes the node pools from host lengths.  No stream's frames / seen / map length change here.
int sskip_front(ctcd_decoder *d, ctcd_stream **states, const float *probs, const int32_t *seq_lens_host, int B, int T, int V, int blank_id,
                int log_input, hipStream_t stream, SkChunk &ck) {
  namespace ss = ctcsskip;
  if (V <= 0 || blank_id < 0 || blank_id >= V) return fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (log_input < 0 || log_input > 2) return fail(CTCD_EINVAL, "log_input is 0, 1 or 2");
  const unsigned long long call_id = ++g_stream_call_id;
  ck.lens.assign((size_t)B, 0);
  ck.kept.assign((size_t)B, 0);
  ck.considered = 0;
  for (int b = 0; b < B; ++b) {
    ctcd_stream *st = states[b];
    if (st->device != d->device || st->V != V) return fail(CTCD_EINVAL, "stream state does not match the decoder configuration");
    if (st->seen_in_call == call_id) return fail(CTCD_EINVAL, "the same stream state appears twice in one batch");
    st->seen_in_call = call_id;
    if (st->seen + T > 0x7fffffffLL) return fail(CTCD_EUNSUPPORTED, "stream too long: the frame map holds 32-bit frame numbers");
    const int len = seq_lens_host ? seq_lens_host[b] : T;
    ck.lens[b] = len < 0 ? 0 : (len > T ? T : len);  // binding.cpp:171
    ck.considered += ck.lens[b];
  }
  ck.rows = probs;
  ck.log_input = log_input;
  ck.dtype = d->in_dtype;
  d->sk_timed = false;
  d->sk_remap_timed = false;
  d->sk_wait_ms = 0.f;
  if (ck.considered == 0) return CTCD_OK;  // no frame to look at: the decode sees B empty chunks
  if (!probs) return fail(CTCD_EINVAL, "null tensor");
  for (int b = 0; b < B; ++b) {  // the maps: room for every frame of the chunk
    ctcd_stream *st = states[b];
    const long long need = ss::map_need(st->frames, ck.lens[b]);
    if (need <= st->map_cap) continue;
    const long long cap = ss::map_grown_cap(st->map_cap, need);
    int32_t *nm = nullptr;
    HIP_TRY(hipMalloc((void **)&nm, (size_t)cap * 4));
    if (st->map && st->frames > 0) {
      const hipError_t ce = hipMemcpyAsync(nm, st->map, (size_t)st->frames * 4, hipMemcpyDeviceToDevice, stream);
      if (ce != hipSuccess) { (void)hipFree(nm); return fail(CTCD_EHIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(ce)); }
    }
    if (st->map) {  // (a remap queued on another stream may still read the old map: hipFree waits for the device)
      const hipError_t se = hipStreamSynchronize(stream);
      if (se != hipSuccess) { (void)hipFree(nm); return fail(CTCD_EHIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(se)); }
      (void)hipFree(st->map);
    }
    st->map = nm;
    st->map_cap = cap;
  }
  int rc;
  char *hb = nullptr, *db = nullptr;
  if ((rc = sskip_region(d, B, &hb, &db))) return rc;
  const SkRegion r(d->h_sk_items);
  ss::StreamSkipItem *h_tab = (ss::StreamSkipItem *)hb;
  int32_t *h_len = (int32_t *)(hb + r.o_len);
  volatile int32_t *h_cnt = (volatile int32_t *)(hb + r.o_cnt);
  for (int b = 0; b < B; ++b) {
    h_tab[b] = ss::StreamSkipItem{states[b]->map, (int32_t)states[b]->frames, (int32_t)states[b]->seen};
    h_len[b] = ck.lens[b];
    h_cnt[b] = -1;  // ("no result": a workgroup that never ran cannot read back as a count)
  }
  const int32_t *d_len = (const int32_t *)(db + r.o_len);
  int32_t *d_cnt = (int32_t *)(db + r.o_cnt);
  const size_t n = (size_t)B * T * V;
  if (d->timing) {
    if ((rc = sskip_timing_events(d))) return rc;
    HIP_TRY(hipEventRecord(d->ev_sk[0], stream));
  }
  const void *rows_in = probs;
  int dt = d->in_dtype;
  float cmp = log_input == 0 ? d->sk_cmp_prob : d->sk_cmp_log;
  if (log_input == 2) {  // raw logits: the float32 log-softmax rows are what the definition compares, and what the decode then reads
    {
      std::lock_guard<std::mutex> lock(d->mu);
      if ((rc = ensure_tables(d))) return rc;
    }
    if ((rc = d->sk_lsm.ensure(n * 4))) return rc;
    if ((rc = launch_log_softmax(d, probs, (float *)d->sk_lsm.p, (long long)B * T, d_len, T, V, stream, dt))) return rc;
    rows_in = d->sk_lsm.p;
    dt = CTCD_DTYPE_F32;
    ck.log_input = 1;
  }
  if ((rc = d->sk_rows.ensure(n * in_elem_bytes(dt))) || (rc = d->sk_kept.ensure((size_t)B * T * 4))) return rc;
  int e = ss::launch_chunk_scan(rows_in, d_len, (const ss::StreamSkipItem *)db, B, T, V, blank_id, cmp, dt, (int32_t *)d->sk_kept.p, d_cnt, (void *)stream);
  if (e != (int)hipSuccess) return fail(CTCD_EHIP, std::string("ctc_stream_scan_kernel: ") + hipGetErrorString((hipError_t)e));
  e = ctcskip::launch_blank_gather(rows_in, d->sk_rows.p, (const int32_t *)d->sk_kept.p, d_cnt, B, T, V, dt, (void *)stream);
  if (e != (int)hipSuccess) {
    (void)hipStreamSynchronize(stream);  // (the scan still writes the region)
    return fail(CTCD_EHIP, std::string("ctc_blank_gather_kernel: ") + hipGetErrorString((hipError_t)e));
  }
  if (d->timing) {
    HIP_TRY(hipEventRecord(d->ev_sk[1], stream));
    d->sk_timed = true;
  }
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipStreamSynchronize(stream));  // the wait for the kept counts
  d->sk_wait_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (int b = 0; b < B; ++b) {
    const int k = h_cnt[b];
    if (k < 0 || k > ck.lens[b]) return fail(CTCD_EINTERNAL, "blank-frame filter: kept count " + std::to_string(k) + " for item " + std::to_string(b));
    ck.kept[b] = k;
  }
  ck.rows = (const float *)d->sk_rows.p;
  ck.dtype = dt;
  return CTCD_OK;
}

// the decode launch was accepted: frames (advanced by the decode), frames seen and the map's used length move together
void sskip_advance(ctcd_decoder *d, ctcd_stream **states, int B, const SkChunk &ck) {
  long long kept = 0;
  for (int b = 0; b < B; ++b) {
    states[b]->seen += ck.lens[b];
    states[b]->filtered = true;
    kept += ck.kept[b];
  }
  d->sk_last[0] = ck.considered;
  d->sk_last[1] = kept;
}

}  // namespace

// Compacts the node pools of B parked streams of one beam width (stream_compact.h), behind whatever is queued on `stream`:
// count -> the host sizes the scratch and decides which streams move to a smaller block -> gather -> store.  The caller has checked
// the states.  live_out (host, or null): nodes of every stream's live set.  Synchronous.
static int compact_streams(ctcd_decoder *d, ctcd_stream **sts, int B, int32_t *live_out, hipStream_t stream) {
  namespace cc = ctccompact;
  std::lock_guard<std::mutex> lock(d->mu);
  const int beam = sts[0]->beam;
  if (cc::compact_lds_bytes(beam) + 1024 > (size_t)d->max_lds)
    return fail(CTCD_EUNSUPPORTED, "stream compaction: the layout arrays of this beam width exceed one workgroup's LDS");
  const size_t n = (size_t)B, o_dst = n * 8, o_scr = 2 * n * 8, o_cap = 3 * n * 8, o_dcap = o_cap + n * 4, o_live = o_dcap + n * 4,
               o_stat = o_live + n * 4, need = o_stat + n * 4;
  if (d->h_cp_cap < need) {
    if (d->h_cp) (void)hipHostFree(d->h_cp);
    d->h_cp = nullptr;
    d->h_cp_cap = 0;
    HIP_TRY(hipHostMalloc((void **)&d->h_cp, 2 * need, hipHostMallocMapped | hipHostMallocCoherent));
    d->h_cp_cap = 2 * need;
  }
  char *hb = d->h_cp, *db = nullptr;
  HIP_TRY(hipHostGetDevicePointer((void **)&db, hb, 0));
  char **h_blk = (char **)hb, **h_dst = (char **)(hb + o_dst);
  long long *h_scr = (long long *)(hb + o_scr);
  int *h_cap = (int *)(hb + o_cap), *h_dcap = (int *)(hb + o_dcap);
  volatile int *h_live = (volatile int *)(hb + o_live), *h_stat = (volatile int *)(hb + o_stat);
  for (int b = 0; b < B; ++b) {
    h_blk[b] = h_dst[b] = sts[b]->block;
    h_cap[b] = h_dcap[b] = (int)cc::pool_capacity(sts[b]->cap_frames, beam);
    h_scr[b] = 0;
    h_live[b] = -1;  // ("no result": a workgroup that never ran cannot read back as a count)
    h_stat[b] = cc::COMPACT_OK;
  }
  cc::CompactLaunch l;
  l.ctl = cc::CompactCtl{(char *const *)db, (const int *)(db + o_cap), (int *)(db + o_live), (int *)(db + o_stat), (char *const *)(db + o_dst),
                         (const int *)(db + o_dcap), (const long long *)(db + o_scr)};
  l.scratch = nullptr;
  l.pool_off = (long long)stream_pool_offset(beam);
  l.B = B; l.K = beam;
  int e = cc::launch_compact_count(l, (void *)stream);
  if (e != (int)hipSuccess) return fail(CTCD_EHIP, std::string("ctc_stream_compact_count_kernel: ") + hipGetErrorString((hipError_t)e));
  HIP_TRY(hipStreamSynchronize(stream));
  long long total = 0;
  for (int b = 0; b < B; ++b) {
    const int M = h_live[b];
    if (M < 0) return fail(CTCD_EINTERNAL, "ctcd_stream_compact: the parked state of item " + std::to_string(b) + " is not one a decode wrote");
    h_scr[b] = total;
    total += (long long)cc::compact_out_ints(M);
  }
  if (total > 0) {
    int rc;
    if ((size_t)total * 4 > d->cp_scratch.cap && (rc = d->cp_scratch.ensure((size_t)total * 4 + (size_t)total)))  // (a quarter of headroom)
      return rc;
    l.scratch = (int *)d->cp_scratch.p;
    // a stream whose live set needs at most a quarter of its block moves to a smaller one: the only allocation of the call
    std::vector<std::pair<char *, long long>> moved((size_t)B, {nullptr, 0});
    auto drop_moved = [&] { for (auto &m : moved) if (m.first) (void)hipFree(m.first); };
    for (int b = 0; b < B; ++b) {
      const int M = h_live[b];
      const long long nf = M > 0 ? cc::shrunk_cap_frames(sts[b]->cap_frames, sts[b]->hint_frames, M, beam) : 0;
      if (!nf) continue;
      char *nb = nullptr;
      const hipError_t me = hipMalloc((void **)&nb, stream_block_bytes(nf, beam));
      if (me != hipSuccess) { drop_moved(); return fail(CTCD_EHIP, std::string("hipMalloc: ") + hipGetErrorString(me)); }
      moved[b] = {nb, nf};
      h_dst[b] = nb;
      h_dcap[b] = (int)cc::pool_capacity(nf, beam);
    }
    e = cc::launch_compact_move(l, (void *)stream);
    if (e == (int)hipSuccess) e = (int)hipStreamSynchronize(stream);
    if (e != (int)hipSuccess) { drop_moved(); return fail(CTCD_EHIP, std::string("ctc_stream_compact kernels: ") + hipGetErrorString((hipError_t)e)); }
    for (int b = 0; b < B; ++b)
      if (h_stat[b] != cc::COMPACT_OK) {
        drop_moved();
        return fail(CTCD_EINTERNAL, "ctcd_stream_compact: status " + std::to_string(h_stat[b]) + " for item " + std::to_string(b));
      }
    for (int b = 0; b < B; ++b) {
      ctcd_stream *st = sts[b];
      const int M = h_live[b];
      if (M <= 0) continue;
      if (moved[b].first) {
        (void)hipFree(st->block);
        st->block = moved[b].first;
        st->cap_frames = moved[b].second;
        st->bytes = stream_block_bytes(st->cap_frames, beam);
      }
      st->base_nodes = M;
      st->base_frames = st->frames;
    }
  }
  if (live_out)
    for (int b = 0; b < B; ++b) live_out[b] = h_live[b] > 0 ? h_live[b] : 1;  // (a stream without frames: the root alone)
  return CTCD_OK;
}

// grows a stream's block so that its pool takes `need` nodes (device-to-device copy of the parked state)
static int stream_grow(ctcd_stream *st, long long need, hipStream_t stream) {
  const int beam = st->beam;
  const long long cap = ctccompact::grown_cap_frames(st->cap_frames, need, beam);
  const size_t bytes = stream_block_bytes(cap, beam);
  char *nb = nullptr;
  HIP_TRY(hipMalloc((void **)&nb, bytes));
  HIP_TRY(hipStreamSynchronize(stream));
  const size_t used = (size_t)ctccompact::pool_bound(st->frames, st->base_nodes, st->base_frames, beam), off = stream_pool_offset(beam);
  HIP_TRY(hipMemcpy(nb, st->block, off + used * sizeof(PoolNode), hipMemcpyDeviceToDevice));
  HIP_TRY(hipMemcpy(nb + off + stream_nodes(cap, beam) * sizeof(PoolNode),
                    st->block + off + stream_nodes(st->cap_frames, beam) * sizeof(PoolNode), used * sizeof(int), hipMemcpyDeviceToDevice));
  HIP_TRY(hipMemset(nb + stream_thi_offset(cap, beam), 0, stream_nodes(cap, beam) * sizeof(int)));
  HIP_TRY(hipMemcpy(nb + stream_thi_offset(cap, beam), st->block + stream_thi_offset(st->cap_frames, beam), used * sizeof(int), hipMemcpyDeviceToDevice));
  (void)hipFree(st->block);
  st->block = nb;
  st->bytes = bytes;
  st->cap_frames = cap;
  return CTCD_OK;
}

// what every streaming call does first: the states are checked against the call, the chunk lengths clamped (binding.cpp:171),
// node pools that the chunk would overflow grown -- or, with ctcd_set_stream_compaction, compacted first and grown only if the
// chunk still does not fit
static int stream_prepare(ctcd_decoder *d, ctcd_stream **states, const unsigned char *is_eos, const int32_t *seq_lens_host, int B, int T, int V,
                          int beam, int out_T, hipStream_t stream, std::vector<int32_t> &lens, bool &any_eos) {
  namespace cc = ctccompact;
  const unsigned long long call_id = ++g_stream_call_id;
  any_eos = false;
  std::vector<ctcd_stream *> compact_first;
  std::vector<int> compact_item;
  for (int b = 0; b < B; ++b) {
    ctcd_stream *st = states[b];
    if (!st || st->V != V || st->beam != beam) return fail(CTCD_EINVAL, "stream state does not match the decoder configuration");
    if (st->scorer != states[0]->scorer) return fail(CTCD_EINVAL, "the streams of one batch must share their scorer");
    if (st->seen_in_call == call_id) return fail(CTCD_EINVAL, "the same stream state appears twice in one batch");
    st->seen_in_call = call_id;
    any_eos |= is_eos[b] != 0;
    int len = seq_lens_host ? seq_lens_host[b] : T;
    len = len < 0 ? 0 : (len > T ? T : len);  // binding.cpp:171
    lens[b] = len;
    if (is_eos[b] && st->frames + len > out_T) return fail(CTCD_EINVAL, "out_T is smaller than the number of frames of a finishing stream");
    // nodes the pool may hold once the chunk is in (frames * beam + 1 for a stream that was never compacted)
    const long long need = cc::pool_bound(st->frames + len, st->base_nodes, st->base_frames, beam);
    const bool fits = need <= cc::pool_capacity(st->cap_frames, beam);
    if (!fits && d->compact_min_nodes > 0 && st->frames > st->base_frames && st->device == d->device &&
        cc::pool_bound(st->frames, st->base_nodes, st->base_frames, beam) >= d->compact_min_nodes) {
      compact_first.push_back(st);
      compact_item.push_back(b);
      continue;
    }
    if (need > 0x7fffffffLL) return fail(CTCD_EUNSUPPORTED, "stream too long for this beam width");
    if (!fits) {
      const int rc = stream_grow(st, need, stream);
      if (rc) return rc;
    }
  }
  if (!compact_first.empty()) {
    int rc = compact_streams(d, compact_first.data(), (int)compact_first.size(), nullptr, stream);
    if (rc) return rc;
    for (size_t i = 0; i < compact_first.size(); ++i) {
      ctcd_stream *st = compact_first[i];
      const long long need = cc::pool_bound(st->frames + lens[compact_item[i]], st->base_nodes, st->base_frames, beam);
      if (need > 0x7fffffffLL) return fail(CTCD_EUNSUPPORTED, "stream too long for this beam width");
      if (need > cc::pool_capacity(st->cap_frames, beam) && (rc = stream_grow(st, need, stream))) return rc;
    }
  }
  return CTCD_OK;
}

int ctcd_stream_compact(ctcd_decoder *d, ctcd_stream **states, int B, int32_t *live_nodes_host, void *stream_) {
  if (!d || B < 0 || (B > 0 && !states)) return fail(CTCD_EINVAL, "bad arguments");
  if (B == 0) return CTCD_OK;
  CTC_ON_DEVICE(d->device);
  const unsigned long long call_id = ++g_stream_call_id;
  for (int b = 0; b < B; ++b) {
    ctcd_stream *st = states[b];
    if (!st || st->device != d->device || st->beam != states[0]->beam || st->V != states[0]->V)
      return fail(CTCD_EINVAL, "stream state does not match the decoder configuration");
    if (st->scorer != states[0]->scorer) return fail(CTCD_EINVAL, "the streams of one batch must share their scorer");
    if (st->seen_in_call == call_id) return fail(CTCD_EINVAL, "the same stream state appears twice in one batch");
    st->seen_in_call = call_id;
  }
  return compact_streams(d, states, B, live_nodes_host, (hipStream_t)stream_);
}

// Commits the final labels of B parked scorer-free streams of one beam width and drops their trunks (stream_commit.h), behind whatever
// is queued on `stream`: count -> the host sizes scratch and results (the allocator is called here) and decides which streams move
// to a smaller block -> gather -> store -> the labels come over.  The caller has checked the states.  Synchronous; shares the
// compaction's scratch and page-locked region.
static int commit_streams(ctcd_decoder *d, ctcd_stream **sts, int B, ctcd_result_alloc_fn alloc, void *alloc_user, int32_t *counts_out,
                          int32_t *live_out, int *out_L, hipStream_t stream, bool filtered) {
  namespace cc = ctccompact;
  namespace cm = ctccommit;
  std::lock_guard<std::mutex> lock(d->mu);
  const int beam = sts[0]->beam;
  if (cc::compact_lds_bytes(beam) + 1024 > (size_t)d->max_lds)
    return fail(CTCD_EUNSUPPORTED, "stream commit: the layout arrays of this beam width exceed one workgroup's LDS");
  const size_t n = (size_t)B, o_dst = n * 8, o_scr = 2 * n * 8, o_lab = 3 * n * 8, o_cap = 4 * n * 8, o_dcap = o_cap + n * 4, o_live = o_dcap + n * 4,
               o_stat = o_live + n * 4, o_drop = o_stat + n * 4, need = o_drop + n * 4;
  if (d->h_cp_cap < need) {
    if (d->h_cp) (void)hipHostFree(d->h_cp);
    d->h_cp = nullptr;
    d->h_cp_cap = 0;
    HIP_TRY(hipHostMalloc((void **)&d->h_cp, 2 * need, hipHostMallocMapped | hipHostMallocCoherent));
    d->h_cp_cap = 2 * need;
  }
  char *hb = d->h_cp, *db = nullptr;
  HIP_TRY(hipHostGetDevicePointer((void **)&db, hb, 0));
  char **h_blk = (char **)hb, **h_dst = (char **)(hb + o_dst);
  long long *h_scr = (long long *)(hb + o_scr), *h_lab = (long long *)(hb + o_lab);
  int *h_cap = (int *)(hb + o_cap), *h_dcap = (int *)(hb + o_dcap);
  volatile int *h_live = (volatile int *)(hb + o_live), *h_stat = (volatile int *)(hb + o_stat), *h_drop = (volatile int *)(hb + o_drop);
  for (int b = 0; b < B; ++b) {
    h_blk[b] = h_dst[b] = sts[b]->block;
    h_cap[b] = h_dcap[b] = (int)cc::pool_capacity(sts[b]->cap_frames, beam);
    h_scr[b] = h_lab[b] = 0;
    h_live[b] = -1;  // ("no result": a workgroup that never ran cannot read back as a count)
    h_drop[b] = 0;
    h_stat[b] = cc::COMPACT_OK;
  }
  cm::CommitLaunch l;
  l.ctl.c = cc::CompactCtl{(char *const *)db, (const int *)(db + o_cap), (int *)(db + o_live), (int *)(db + o_stat), (char *const *)(db + o_dst),
                           (const int *)(db + o_dcap), (const long long *)(db + o_scr)};
  l.ctl.drop = (int *)(db + o_drop);
  l.ctl.lab = (const long long *)(db + o_lab);
  l.scratch = nullptr;
  l.pool_off = (long long)stream_pool_offset(beam);
  l.B = B; l.K = beam;
  int e = cm::launch_commit_count(l, (void *)stream);
  if (e != (int)hipSuccess) return fail(CTCD_EHIP, std::string("ctc_stream_commit_count_kernel: ") + hipGetErrorString((hipError_t)e));
  HIP_TRY(hipStreamSynchronize(stream));
  long long total = 0, labels = 0;
  int L = 0, bad = -1;
  for (int b = 0; b < B; ++b) {
    const int M = h_live[b], D = h_drop[b];
    if (M < 0 || D < 0 || (M > 0 && D >= M))
      return fail(CTCD_EINTERNAL, "ctcd_stream_commit: the parked state of item " + std::to_string(b) + " is not one a decode wrote");
    h_scr[b] = total;
    total += (long long)cc::compact_out_ints(M > 0 ? M - D : 0);
    L = D > L ? D : L;
  }
  for (int b = 0; b < B; ++b) {  // the labels behind the layouts: tokens, then time steps, per stream
    h_lab[b] = total + labels;
    labels += 2LL * h_drop[b];
  }
  int32_t *r_tok = nullptr, *r_ts = nullptr;
  if (alloc(alloc_user, 1, L, &r_tok, &r_ts) != 0) return fail(CTCD_EINVAL, "the result allocator failed");
  if (L > 0 && (!r_tok || !r_ts)) return fail(CTCD_EINVAL, "the result allocator returned no buffers");
  if (total > 0) {
    int rc;
    const size_t want = (size_t)(total + labels) * 4;
    if (want > d->cp_scratch.cap && (rc = d->cp_scratch.ensure(want + want / 4)))  // (a quarter of headroom)
      return rc;
    l.scratch = (int *)d->cp_scratch.p;
    // a stream whose live set needs at most a quarter of its block moves to a smaller one: the only allocation of the call
    std::vector<std::pair<char *, long long>> moved((size_t)B, {nullptr, 0});
    auto drop_moved = [&] { for (auto &m : moved) if (m.first) (void)hipFree(m.first); };
    for (int b = 0; b < B; ++b) {
      const int M = h_live[b] > 0 ? h_live[b] - h_drop[b] : 0;
      const long long nf = M > 0 ? cc::shrunk_cap_frames(sts[b]->cap_frames, sts[b]->hint_frames, M, beam) : 0;
      if (!nf) continue;
      char *nb = nullptr;
      const hipError_t me = hipMalloc((void **)&nb, stream_block_bytes(nf, beam));
      if (me != hipSuccess) { drop_moved(); return fail(CTCD_EHIP, std::string("hipMalloc: ") + hipGetErrorString(me)); }
      moved[b] = {nb, nf};
      h_dst[b] = nb;
      h_dcap[b] = (int)cc::pool_capacity(nf, beam);
    }
    e = cm::launch_commit_move(l, (void *)stream);
    if (e == (int)hipSuccess) e = (int)hipStreamSynchronize(stream);
    if (e != (int)hipSuccess) { drop_moved(); return fail(CTCD_EHIP, std::string("ctc_stream_commit kernels: ") + hipGetErrorString((hipError_t)e)); }
    std::vector<int32_t> lab((size_t)labels);
    if (labels > 0 && filtered) {
      // filtered streams (stream_blank_skip.h; the caller holds d->mu_skip): the committed time steps, D words behind every stream's D
      // tokens, go back through the maps on the device before they come over
      ctcsskip::StreamRemapItem *h_tab = nullptr;
      const ctcsskip::StreamRemapItem *d_tab = nullptr;
      int rc = sskip_remap_table(d, B, &h_tab, &d_tab);
      if (rc) { drop_moved(); return rc; }
      for (int b = 0; b < B; ++b)
        h_tab[b] = ctcsskip::StreamRemapItem{sts[b]->map, l.scratch + h_lab[b] + (h_drop[b] > 0 ? h_drop[b] : 0), (int32_t)sts[b]->frames, 0};
      e = ctcsskip::launch_remap_rows(nullptr, (const int32_t *)(db + o_drop), nullptr, d_tab, B, 1, L, (void *)stream);
      if (e == (int)hipSuccess) e = (int)hipStreamSynchronize(stream);
      if (e != (int)hipSuccess) { drop_moved(); return fail(CTCD_EHIP, std::string("ctc_stream_remap_rows_kernel: ") + hipGetErrorString((hipError_t)e)); }
    }
    if (labels > 0) {
      const hipError_t ce = hipMemcpy(lab.data(), l.scratch + total, (size_t)labels * 4, hipMemcpyDeviceToHost);
      if (ce != hipSuccess) { drop_moved(); return fail(CTCD_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(ce)); }
    }
    for (int b = 0; b < B; ++b) {
      ctcd_stream *st = sts[b];
      const int M = h_live[b], D = h_drop[b];
      if (M <= 0) continue;
      if (h_stat[b] != cc::COMPACT_OK) {  // a walk left the pool: that stream's block is as it was, nothing of it is committed
        if (bad < 0) bad = b;
        if (moved[b].first) (void)hipFree(moved[b].first);
        h_drop[b] = 0;
        h_live[b] = -1;
        continue;
      }
      if (moved[b].first) {
        (void)hipFree(st->block);
        st->block = moved[b].first;
        st->cap_frames = moved[b].second;
        st->bytes = stream_block_bytes(st->cap_frames, beam);
      }
      st->base_nodes = M - D;
      st->base_frames = st->frames;
      st->committed += D;
      const int32_t *src = lab.data() + (h_lab[b] - total);
      for (int i = 0; i < D; ++i) { r_tok[(size_t)b * L + i] = src[i]; r_ts[(size_t)b * L + i] = src[D + i]; }
    }
  }
  for (int b = 0; b < B; ++b) {
    const int D = h_live[b] > 0 ? h_drop[b] : 0;
    for (int i = D; i < L; ++i) { r_tok[(size_t)b * L + i] = 0; r_ts[(size_t)b * L + i] = 0; }
    counts_out[b] = D;
    if (live_out) live_out[b] = h_live[b] > 0 ? h_live[b] - h_drop[b] : (h_live[b] == 0 ? 1 : -1);  // (a stream without frames: the root alone)
  }
  if (out_L) *out_L = L;
  if (bad >= 0) return fail(CTCD_EINTERNAL, "ctcd_stream_commit: the parked state of item " + std::to_string(bad) + " is not one a decode wrote (it is unchanged)");
  return CTCD_OK;
}

int ctcd_stream_commit(ctcd_decoder *d, ctcd_stream **states, int B, ctcd_result_alloc_fn alloc, void *alloc_user, int32_t *counts_host,
                       int32_t *live_nodes_host, int *out_L, void *stream_) {
  if (!d || B < 0 || (B > 0 && (!states || !alloc || !counts_host))) return fail(CTCD_EINVAL, "bad arguments");
  if (out_L) *out_L = 0;
  if (B == 0) return CTCD_OK;
  CTC_ON_DEVICE(d->device);
  const unsigned long long call_id = ++g_stream_call_id;
  for (int b = 0; b < B; ++b) {
    ctcd_stream *st = states[b];
    if (!st || st->device != d->device || st->beam != states[0]->beam || st->V != states[0]->V)
      return fail(CTCD_EINVAL, "stream state does not match the decoder configuration");
    if (st->scorer != states[0]->scorer) return fail(CTCD_EINVAL, "the streams of one batch must share their scorer");
    if (st->seen_in_call == call_id) return fail(CTCD_EINVAL, "the same stream state appears twice in one batch");
    st->seen_in_call = call_id;
  }
  // (with a scorer the result scores use a prefix's absolute depth -- finish(), lm_final_scores: a re-rooted stream would need a base depth there)
  if (states[0]->scorer) return fail(CTCD_EUNSUPPORTED, "ctcd_stream_commit: streams with a scorer cannot drop their trunk");
  if (const int src = sskip_check_setting(d, states, B, "ctcd_stream_commit")) return src;
  // (the blank-frame filter of live streams: its lock is taken before the decoder's, as a filtered chunk call takes them)
  std::unique_lock<std::mutex> sk_lock(d->mu_skip, std::defer_lock);
  if (d->sk_on) sk_lock.lock();
  return commit_streams(d, states, B, alloc, alloc_user, counts_host, live_nodes_host, out_L, (hipStream_t)stream_, sk_lock.owns_lock());
}

long long ctcd_stream_committed(const ctcd_stream *st) { return st ? st->committed : -1; }

// ---- images of live streams (stream_snapshot.h) -----------------------------------------------------------------------------------
// the decoder's page-locked region (shared with the compaction and the commit) with room for `need` bytes
static int snap_region(ctcd_decoder *d, size_t need, char **hb, char **db) {
  if (d->h_cp_cap < need) {
    if (d->h_cp) (void)hipHostFree(d->h_cp);
    d->h_cp = nullptr;
    d->h_cp_cap = 0;
    HIP_TRY(hipHostMalloc((void **)&d->h_cp, 2 * need, hipHostMallocMapped | hipHostMallocCoherent));
    d->h_cp_cap = 2 * need;
  }
  *hb = d->h_cp;
  HIP_TRY(hipHostGetDevicePointer((void **)db, *hb, 0));
  return CTCD_OK;
}
// offsets of the per-stream arrays in that region: blocks | image offsets | meta | pool capacities | node counts
struct SnapRegion {
  size_t o_off, o_meta, o_cap, o_nodes, need;
  explicit SnapRegion(size_t n) {
    o_off = n * 8;
    o_meta = 2 * n * 8;
    o_cap = o_meta + n * sizeof(ctcsnap::SnapMeta);
    o_nodes = o_cap + n * 4;
    need = o_nodes + n * 4;
  }
};

int ctcd_stream_save(ctcd_decoder *d, ctcd_stream **states, int B, ctcd_bytes_alloc_fn alloc, void *alloc_user, unsigned long long *bytes_out,
                     void *stream_) {
  namespace sn = ctcsnap;
  if (!d || B < 0 || (B > 0 && (!states || !alloc || !bytes_out))) return fail(CTCD_EINVAL, "bad arguments");
  if (B == 0) return CTCD_OK;
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned long long call_id = ++g_stream_call_id;
  for (int b = 0; b < B; ++b) {
    ctcd_stream *st = states[b];
    if (!st || st->device != d->device || st->beam != states[0]->beam || st->V != states[0]->V)
      return fail(CTCD_EINVAL, "stream state does not match the decoder configuration");
    if (st->scorer != states[0]->scorer) return fail(CTCD_EINVAL, "the streams of one batch must share their scorer");
    if (st->seen_in_call == call_id) return fail(CTCD_EINVAL, "the same stream state appears twice in one batch");
    st->seen_in_call = call_id;
  }
  const ctcd_scorer *sc = states[0]->scorer;
  if (sc && sc->cbl) return fail(CTCD_EUNSUPPORTED, "ctcd_stream_save: the states of a stream behind a callback scorer index a per-process cache");
  for (int b = 0; b < B; ++b)
    if (states[b]->filtered && states[b]->seen > 0)
      return fail(CTCD_EUNSUPPORTED, "ctcd_stream_save: item " + std::to_string(b) + " decodes behind the blank-frame filter (an image does not hold its frame map)");
  const int beam = states[0]->beam, lm = sc ? 1 : 0;
  // the image is the layout a compaction leaves
  std::vector<int32_t> live((size_t)B, 0);
  int rc = compact_streams(d, states, B, live.data(), stream);
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(d->mu);
  const SnapRegion r((size_t)B);
  char *hb = nullptr, *db = nullptr;
  if ((rc = snap_region(d, r.need, &hb, &db))) return rc;
  char **h_blk = (char **)hb;
  long long *h_off = (long long *)(hb + r.o_off);
  sn::SnapMeta *h_meta = (sn::SnapMeta *)(hb + r.o_meta);
  int *h_cap = (int *)(hb + r.o_cap), *h_nodes = (int *)(hb + r.o_nodes);
  size_t total = 0;
  for (int b = 0; b < B; ++b) {
    const ctcd_stream *st = states[b];
    const int M = st->frames > 0 ? live[b] : 1;
    if (M < 1 || (long long)M > ctccompact::pool_capacity(st->cap_frames, beam))
      return fail(CTCD_EINTERNAL, "ctcd_stream_save: node count " + std::to_string(M) + " for item " + std::to_string(b));
    h_blk[b] = st->block;
    h_cap[b] = (int)ctccompact::pool_capacity(st->cap_frames, beam);
    h_nodes[b] = M;
    h_off[b] = (long long)(total / 4);
    h_meta[b] = sn::SnapMeta{st->frames, st->committed, sc ? sc->fingerprint : 0ull, st->V, lm ? sn::SNAP_SCORER_BUILTIN : sn::SNAP_SCORER_NONE};
    bytes_out[b] = sn::snapshot_bytes(beam, lm, M);
    total += sn::snapshot_padded((size_t)bytes_out[b]);
  }
  void *host = alloc(alloc_user, (unsigned long long)total);
  if (!host) return fail(CTCD_EINVAL, "the image allocator returned no buffer");
  if (total > d->cp_scratch.cap && (rc = d->cp_scratch.ensure(total + total / 4))) return rc;
  sn::SnapLaunch l;
  l.ctl = sn::SnapCtl{(char *const *)db, (const int *)(db + r.o_cap), (const int *)(db + r.o_nodes), (const long long *)(db + r.o_off),
                      (const sn::SnapMeta *)(db + r.o_meta)};
  l.staging = (int *)d->cp_scratch.p;
  l.pool_off = (long long)stream_pool_offset(beam);
  l.B = B; l.K = beam;
  HIP_TRY(hipMemsetAsync(l.staging, 0, total, stream));  // (the padding between images travels as zero)
  const int e = sn::launch_snapshot_export(l, (void *)stream);
  if (e != (int)hipSuccess) return fail(CTCD_EHIP, std::string("ctc_stream_export_kernel: ") + hipGetErrorString((hipError_t)e));
  HIP_TRY(hipMemcpyAsync(host, l.staging, total, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return CTCD_OK;
}

int ctcd_snapshot_info(const void *blob, unsigned long long bytes, ctcd_snapshot_info_t *info) {
  if (!blob || !info || bytes == 0) return fail(CTCD_EINVAL, "ctcd_snapshot_info: bad arguments");
  ctcsnap::SnapInfo in;
  const int c = ctcsnap::snapshot_info(blob, (size_t)bytes, &in);
  if (c != ctcsnap::SNAP_OK) return fail(CTCD_EINVAL, std::string("not a stream image: ") + ctcsnap::snapshot_error_name(c));
  info->version = in.version; info->beam = in.beam; info->labels = in.labels; info->scorer_kind = in.scorer_kind; info->nodes = in.nodes;
  info->reserved = 0; info->frames = in.frames; info->committed = in.committed; info->fingerprint = in.fingerprint; info->bytes = in.bytes;
  return CTCD_OK;
}

unsigned long long ctcd_scorer_fingerprint(const ctcd_scorer *s) { return s && !s->cbl ? s->fingerprint : 0ull; }

int ctcd_stream_restore(ctcd_decoder *d, ctcd_scorer *scorer, const void *const *blobs, const unsigned long long *bytes, int B, int frames_hint,
                        ctcd_stream **out, void *stream_) {
  namespace sn = ctcsnap;
  namespace cc = ctccompact;
  if (!d || B < 0 || frames_hint < 0 || (B > 0 && (!blobs || !bytes || !out))) return fail(CTCD_EINVAL, "bad arguments");
  if (B == 0) return CTCD_OK;
  for (int b = 0; b < B; ++b) {
    out[b] = nullptr;
    if (!blobs[b] || bytes[b] == 0) return fail(CTCD_EINVAL, "ctcd_stream_restore: item " + std::to_string(b) + " is empty");
  }
  if (scorer && scorer->cbl) return fail(CTCD_EUNSUPPORTED, "ctcd_stream_restore: no image is saved behind a callback scorer");
  if (d->sk_on) return fail(CTCD_EUNSUPPORTED, "ctcd_stream_restore: this decoder has the blank-frame filter of live streams on (an image holds no frame map)");
  if (scorer && scorer->device != d->device) return fail(CTCD_EINVAL, "the scorer lives on another device than the decoder");
  // every image is checked before anything is allocated or uploaded
  sn::SnapInfo first;
  {
    const int c = sn::snapshot_info(blobs[0], (size_t)bytes[0], &first);
    if (c != sn::SNAP_OK) return fail(CTCD_EINVAL, std::string("ctcd_stream_restore: item 0 is refused: ") + sn::snapshot_error_name(c));
  }
  sn::SnapExpect ex;
  ex.K = first.beam; ex.V = first.labels;
  ex.scorer_kind = scorer ? sn::SNAP_SCORER_BUILTIN : sn::SNAP_SCORER_NONE;
  ex.fingerprint = scorer ? scorer->fingerprint : 0ull;
  ex.lm_states = scorer ? (long long)scorer->host.st_bo.size() : 0;
  ex.lm_dict = scorer ? (long long)scorer->host.dict.size() : 0;
  ex.lm_dict_lab = scorer ? (long long)scorer->host.dict_lab.size() : 0;
  ex.lm_char_based = scorer && scorer->host.char_based ? 1 : 0;
  ex.lm_dict_wide = scorer ? scorer->dview.dict_wide : 0;
  if (ex.V < 1 || ex.V > kMaxVocab) return fail(CTCD_EINVAL, "ctcd_stream_restore: item 0 is refused: label count");
  if (scorer && (size_t)ex.V != scorer->host.labels.size()) return fail(CTCD_EINVAL, "ctcd_stream_restore: item 0 is refused: label count against the scorer");
  const int beam = ex.K, lm = scorer ? 1 : 0;
  std::vector<int> nodes((size_t)B);
  std::vector<long long> frames((size_t)B), committed((size_t)B);
  size_t total = 0;
  // (the check reads every word of every image: a large batch is shared among a few threads)
  std::vector<sn::SnapError> errs((size_t)B);
  {
    unsigned long long all = 0;
    for (int b = 0; b < B; ++b) all += bytes[b];
    const int nth = all < (4ull << 20) ? 1 : (B < 8 ? B : 8);
    auto run = [&](int t) { for (int b = t; b < B; b += nth) (void)sn::snapshot_check(blobs[b], (size_t)bytes[b], ex, &errs[(size_t)b]); };
    std::vector<std::thread> th;
    for (int t = 1; t < nth; ++t) th.emplace_back(run, t);
    run(0);
    for (auto &t : th) t.join();
  }
  for (int b = 0; b < B; ++b) {
    const sn::SnapError &err = errs[(size_t)b];
    if (err.code != sn::SNAP_OK)
      return fail(CTCD_EINVAL, "ctcd_stream_restore: item " + std::to_string(b) + " is refused: " + sn::snapshot_error_name(err.code) +
                                   (err.at >= 0 ? " (at " + std::to_string(err.at) + ")" : std::string()));
    sn::SnapInfo in;
    (void)sn::snapshot_info(blobs[b], (size_t)bytes[b], &in);
    nodes[b] = in.nodes; frames[b] = in.frames; committed[b] = in.committed;
    total += sn::snapshot_padded((size_t)bytes[b]);
  }
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  std::lock_guard<std::mutex> lock(d->mu);
  // capacities as after a compaction that left M nodes: max(capacity of the hint, 2 * M) nodes in whole frames
  const long long hint = frames_hint > 0 ? frames_hint : 1024;
  std::vector<ctcd_stream *> made;
  auto drop = [&] { for (ctcd_stream *st : made) { if (st->block) (void)hipFree(st->block); delete st; } };
  for (int b = 0; b < B; ++b) {
    const long long for_2m = (2LL * nodes[b] - 1 + beam - 1) / beam;
    ctcd_stream *st = new ctcd_stream;
    made.push_back(st);
    st->device = d->device; st->scorer = scorer; st->V = ex.V; st->beam = beam;
    st->frames = frames[b]; st->committed = committed[b];
    st->hint_frames = hint;
    st->cap_frames = hint > for_2m ? hint : for_2m;
    if (frames[b] > 0) { st->base_nodes = nodes[b]; st->base_frames = frames[b]; }
    if (cc::pool_capacity(st->cap_frames, beam) > 0x7fffffffLL) { drop(); return fail(CTCD_EUNSUPPORTED, "stream too long for this beam width"); }
    st->bytes = stream_block_bytes(st->cap_frames, beam);
    const hipError_t me = hipMalloc((void **)&st->block, st->bytes);
    if (me != hipSuccess) { st->block = nullptr; drop(); return fail(CTCD_EHIP, std::string("hipMalloc: ") + hipGetErrorString(me)); }
  }
  int rc;
  const SnapRegion r((size_t)B);
  char *hb = nullptr, *db = nullptr;
  if ((rc = snap_region(d, r.need, &hb, &db))) { drop(); return rc; }
  if (total > d->cp_scratch.cap && (rc = d->cp_scratch.ensure(total + total / 4))) { drop(); return rc; }
  char **h_blk = (char **)hb;
  long long *h_off = (long long *)(hb + r.o_off);
  int *h_cap = (int *)(hb + r.o_cap), *h_nodes = (int *)(hb + r.o_nodes);
  // one copy brings every image in: straight from the caller's memory where the images lie as ctcd_stream_save laid them out (one
  // allocation, each at the next multiple of 16 bytes), else from a packed copy
  bool as_saved = ((uintptr_t)blobs[0] & 3) == 0;
  size_t at = 0;
  for (int b = 0; b < B; ++b) {
    h_blk[b] = made[b]->block;
    h_cap[b] = (int)cc::pool_capacity(made[b]->cap_frames, beam);
    h_nodes[b] = nodes[b];
    h_off[b] = (long long)(at / 4);
    as_saved = as_saved && (const char *)blobs[b] == (const char *)blobs[0] + at;
    at += sn::snapshot_padded((size_t)bytes[b]);
  }
  const size_t span = total - (sn::snapshot_padded((size_t)bytes[B - 1]) - (size_t)bytes[B - 1]);  // (nothing behind the last image is read)
  std::vector<char> pack;
  if (!as_saved) {
    pack.assign(total, 0);
    for (int b = 0; b < B; ++b) memcpy(pack.data() + (size_t)h_off[b] * 4, blobs[b], (size_t)bytes[b]);
  }
  sn::SnapLaunch l;
  l.ctl = sn::SnapCtl{(char *const *)db, (const int *)(db + r.o_cap), (const int *)(db + r.o_nodes), (const long long *)(db + r.o_off),
                      (const sn::SnapMeta *)(db + r.o_meta)};
  l.staging = (int *)d->cp_scratch.p;
  l.pool_off = (long long)stream_pool_offset(beam);
  l.B = B; l.K = beam;
  (void)lm;
  hipError_t e = hipMemcpyAsync(l.staging, as_saved ? blobs[0] : (const void *)pack.data(), span, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) e = (hipError_t)sn::launch_snapshot_import(l, (void *)stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { drop(); return fail(CTCD_EHIP, std::string("ctc_stream_import_kernel: ") + hipGetErrorString(e)); }
  for (int b = 0; b < B; ++b) out[b] = made[b];
  return CTCD_OK;
}

long long ctcd_stream_pool_nodes(const ctcd_stream *st) {
  return st ? ctccompact::pool_bound(st->frames, st->base_nodes, st->base_frames, st->beam) : -1;
}
long long ctcd_stream_pool_capacity(const ctcd_stream *st) { return st ? ctccompact::pool_capacity(st->cap_frames, st->beam) : -1; }
long long ctcd_stream_bytes(const ctcd_stream *st) { return st ? (long long)st->bytes : -1; }

int ctcd_set_stream_compaction(ctcd_decoder *d, long long min_nodes) {
  if (!d || min_nodes < 0) return fail(CTCD_EINVAL, "the compaction threshold is a node count (0: off)");
  d->compact_min_nodes = min_nodes;
  return CTCD_OK;
}

static int stream_decode_impl(ctcd_decoder *d, ctcd_stream **states, const unsigned char *is_eos, const float *probs, const int32_t *seq_lens_host, int B,
                              int T, int V, int beam, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input, int32_t *out_tok,
                              int32_t *out_ts, float *out_sc, int32_t *out_len, int32_t *n_results, int out_T, void *stream_, int in_dtype = -1);

int ctcd_stream_decode(ctcd_decoder *d, ctcd_stream **states, const unsigned char *is_eos, const float *probs,
                       const int32_t *seq_lens_host, int B, int T, int V, int beam, int /*num_processes*/, double cutoff_prob,
                       int cutoff_top_n, int blank_id, int log_input, int32_t *out_tok, int32_t *out_ts, float *out_sc,
                       int32_t *out_len, int32_t *n_results, int out_T, void *stream_) {
  if (!d || !states || !is_eos || B < 0 || T < 0 || out_T < 0) return fail(CTCD_EINVAL, "bad arguments");
  if (B == 0) return CTCD_OK;
  int rc;
  if ((rc = sskip_check_setting(d, states, B, "ctcd_stream_decode"))) return rc;
  if (!d->sk_on)
    return stream_decode_impl(d, states, is_eos, probs, seq_lens_host, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, out_tok, out_ts, out_sc,
                              out_len, n_results, out_T, stream_);
  // the filter is on: scan and gather, the wait for the kept counts, the decode of the kept rows, the remap of what the call reports
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  std::lock_guard<std::mutex> sk_lock(d->mu_skip);
  SkChunk ck;
  if ((rc = sskip_front(d, states, probs, seq_lens_host, B, T, V, blank_id, log_input, stream, ck))) return rc;
  // (the kept rows' element type travels with the call: raw logits are filtered, and decoded, as float32 rows)
  rc = stream_decode_impl(d, states, is_eos, ck.rows, ck.kept.data(), B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, ck.log_input, out_tok, out_ts,
                          out_sc, out_len, n_results, out_T, stream_, ck.dtype);
  if (rc) return rc;
  sskip_advance(d, states, B, ck);
  bool any_eos = false;
  for (int b = 0; b < B; ++b) any_eos |= is_eos[b] != 0;
  if (any_eos && out_ts && out_len && out_T > 0) return sskip_remap_rows(d, states, B, out_ts, out_len, nullptr, beam, out_T, stream);
  return CTCD_OK;
}

static int stream_decode_impl(ctcd_decoder *d, ctcd_stream **states, const unsigned char *is_eos, const float *probs, const int32_t *seq_lens_host, int B,
                              int T, int V, int beam, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input, int32_t *out_tok,
                              int32_t *out_ts, float *out_sc, int32_t *out_len, int32_t *n_results, int out_T, void *stream_, int in_dtype) {
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<int32_t> lens(B);
  bool any_eos = false;
  {
    const int prc = stream_prepare(d, states, is_eos, seq_lens_host, B, T, V, beam, out_T, stream, lens, any_eos);
    if (prc) return prc;
  }
  // (the chunk lengths travel with the other per-item arguments: decode_common)
  if (states[0]->scorer && states[0]->scorer->cbl) {  // a callback scorer: as many launches as its cache needs
    const int rc = cb_rounds(d, states, is_eos, lens.data(), probs, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, states[0]->scorer, out_tok,
                             out_ts, out_sc, out_len, n_results, out_T, stream_, nullptr, false, in_dtype);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) states[b]->frames += lens[b];
    return CTCD_OK;
  }
  StreamCall sc{states, is_eos, out_T, lens.data(), any_eos};
  sc.in_dtype = in_dtype;
  int rc = decode_common(d, probs, nullptr, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, out_tok,
                         out_ts, out_sc, out_len, n_results, stream_, &sc, states[0]->scorer);
  if (rc) return rc;
  for (int b = 0; b < B; ++b) states[b]->frames += lens[b];
  return CTCD_OK;
}

// Interim results of live streams (stream_peek.h): one launch of ctc_stream_peek_kernel on the parked states, behind whatever chunks
// are queued on `stream`.  Everything is refused before anything is queued.
int ctcd_stream_peek(ctcd_decoder *d, ctcd_stream **states, int B, int n_best, const int32_t *since_host, int32_t *out_tok, int32_t *out_ts,
                     int L_cap, float *out_sc, int32_t *out_len, int32_t *n_results, int32_t *stable_lens, void *stream_) {
  if (!d || B < 0 || L_cap < 0 || (B > 0 && !states)) return fail(CTCD_EINVAL, "bad arguments");
  if (B == 0) return CTCD_OK;
  if (!out_sc || !out_len || !n_results || !stable_lens || (L_cap > 0 && (!out_tok || !out_ts))) return fail(CTCD_EINVAL, "null tensor");
  if (n_best < 1) return fail(CTCD_EINVAL, "n_best must be at least 1");
  if (const int src = sskip_check_setting(d, states, B, "ctcd_stream_peek")) return src;
  // (the blank-frame filter of live streams: its lock is taken before the decoder's, as a filtered chunk call takes them)
  std::unique_lock<std::mutex> sk_lock(d->mu_skip, std::defer_lock);
  if (d->sk_on) sk_lock.lock();
  std::lock_guard<std::mutex> lock(d->mu);
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  const unsigned long long call_id = ++g_stream_call_id;
  for (int b = 0; b < B; ++b) {
    ctcd_stream *st = states[b];
    if (!st || st->device != d->device || st->beam != states[0]->beam || st->V != states[0]->V)
      return fail(CTCD_EINVAL, "stream state does not match the decoder configuration");
    if (st->scorer != states[0]->scorer) return fail(CTCD_EINVAL, "the streams of one batch must share their scorer");
    if (st->seen_in_call == call_id) return fail(CTCD_EINVAL, "the same stream state appears twice in one batch");
    st->seen_in_call = call_id;
  }
  const int beam = states[0]->beam;
  ctcd_scorer *scorer = states[0]->scorer;
  if (n_best > beam) return fail(CTCD_EINVAL, "n_best is larger than the beam width");
  if (scorer && scorer->cbl)
    return fail(CTCD_EUNSUPPORTED, "interim results of streams behind a callback scorer (the scorer's cache may not hold the \"<s>\" / \"</s>\" / last-word windows they need)");
  if (scorer && scorer->device != d->device) return fail(CTCD_EINVAL, "the scorer's tables live on another device than the decoder");
  const size_t lds = ctcpeek::peek_lds_bytes(beam, scorer != nullptr);
  if (lds + 1024 > (size_t)d->max_lds) return fail(CTCD_EUNSUPPORTED, "interim results: the sort words of this beam width exceed one workgroup's LDS");
  int rc;
  const size_t off_cap = (size_t)B * 8, off_since = off_cap + (size_t)B * 4, need = (off_since + (size_t)B * 4 + 31) & ~(size_t)15;
  if ((rc = d->peek_args.ensure(2 * need))) return rc;
  if ((rc = d->peek_status.ensure((size_t)B * 4))) return rc;
  if (d->h_pkargs_cap < need) {
    for (int i = 0; i < 2; ++i) {
      if (d->ev_pkargs[i]) HIP_TRY(hipEventSynchronize(d->ev_pkargs[i]));
      if (d->h_pkargs[i]) (void)hipHostFree(d->h_pkargs[i]);
      d->h_pkargs[i] = nullptr;
      HIP_TRY(hipHostMalloc((void **)&d->h_pkargs[i], need, hipHostMallocDefault));
      if (!d->ev_pkargs[i]) HIP_TRY(hipEventCreateWithFlags(&d->ev_pkargs[i], hipEventDisableTiming));
    }
    d->h_pkargs_cap = need;
  }
  const int slot = (int)(d->peek_calls++ & 1);
  HIP_TRY(hipEventSynchronize(d->ev_pkargs[slot]));  // (the copy of two calls ago: long done)
  char *hb = d->h_pkargs[slot];
  for (int b = 0; b < B; ++b) {
    ctcd_stream *st = states[b];
    ((char **)hb)[b] = st->block;
    ((int *)(hb + off_cap))[b] = (int)(st->cap_frames * beam + 1);
    ((int *)(hb + off_since))[b] = since_host ? since_host[b] : 0;
  }
  char *db = (char *)d->peek_args.p + (size_t)slot * need;
  HIP_TRY(hipMemcpyAsync(db, hb, off_since + (size_t)B * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(d->ev_pkargs[slot], stream));
  // every status word starts as -1 ("no result"): a workgroup that never ran cannot read back as ok
  HIP_TRY(hipMemsetAsync(d->peek_status.p, 0xff, (size_t)B * 4, stream));
  ctclm::LmView lmv;
  if (scorer) {
    lmv = scorer->dview;
    lmv.alpha = scorer->host.alpha;  // reset_params takes effect at the next call, as for a decode
    lmv.beta = scorer->host.beta;
  }
  ctcpeek::PeekLaunch l;
  l.blocks = (char *const *)db; l.pool_caps = (const int *)(db + off_cap); l.since = (const int *)(db + off_since);
  l.pool_off = (long long)stream_pool_offset(beam);
  l.B = B; l.K = beam;
  l.lm = scorer ? &lmv : nullptr;
  l.out = ctcpeek::PeekOut{out_tok, out_ts, out_sc, out_len, n_results, stable_lens, n_best, L_cap};
  l.status = (int32_t *)d->peek_status.p;
  const int e = ctcpeek::launch_stream_peek(l, stream_);
  if (e != (int)hipSuccess) return fail(CTCD_EHIP, std::string("ctc_stream_peek_kernel: ") + hipGetErrorString((hipError_t)e));
  d->peek_items = B;
  d->peek_stream = stream;
  // filtered streams report the kept frames' indices among the seen frames: the reported part of every row goes through the maps
  if (sk_lock.owns_lock() && L_cap > 0) return sskip_remap_rows(d, states, B, out_ts, out_len, l.since, n_best, L_cap, stream);
  return CTCD_OK;
}

// The streaming call with its results delivered to HOST memory, sized as the reference sizes them (binding.cpp:186-205: tokens /
// timesteps [B, R, L] with R = the most results of any item that ended, L = the longest of their label sequences).  R and L are
// known only when the kernel has run: the caller hands over an allocator, called once with (R, L), that returns the two buffers
// (the reference's binding resizes its tensors at that point).  The results leave the GPU in compact form -- the kernel mirrors
// every finished stream's records into page-locked memory -- and host threads expand them into the caller's buffers: a tenth of the
// padded [B, K, out_T] pair crosses PCIe.  out_scores / out_lens [B, beam] and n_results [B] are host pointers too.  Synchronous.
// A callback scorer decodes launch after launch into padded device tensors (cb_rounds): not through this entry (CTCD_EUNSUPPORTED).
// (remap_tab, device memory, non-null: the call's streams are filtered -- stream_blank_skip.h; launched(): the decode launch was accepted)
static int stream_decode_to_host_impl(ctcd_decoder *d, ctcd_stream **states, const unsigned char *is_eos, const float *probs,
                                      const int32_t *seq_lens_host, int B, int T, int V, int beam, int num_processes, double cutoff_prob,
                                      int cutoff_top_n, int blank_id, int log_input, ctcd_result_alloc_fn alloc, void *alloc_user,
                                      float *out_sc, int32_t *out_len, int32_t *n_results, int out_T, int *out_R, int *out_L, void *stream_,
                                      const ctcsskip::StreamRemapItem *remap_tab, const std::function<void()> &launched = nullptr, int in_dtype = -1);

int ctcd_stream_decode_to_host(ctcd_decoder *d, ctcd_stream **states, const unsigned char *is_eos, const float *probs,
                               const int32_t *seq_lens_host, int B, int T, int V, int beam, int num_processes, double cutoff_prob,
                               int cutoff_top_n, int blank_id, int log_input, ctcd_result_alloc_fn alloc, void *alloc_user,
                               float *out_sc, int32_t *out_len, int32_t *n_results, int out_T, int *out_R, int *out_L, void *stream_) {
  if (!d || !states || !is_eos || !alloc || !out_sc || !out_len || !n_results || B < 0 || T < 0 || out_T < 0) return fail(CTCD_EINVAL, "bad arguments");
  if (out_R) *out_R = 0;
  if (out_L) *out_L = 0;
  if (B == 0) return CTCD_OK;
  int rc;
  if ((rc = sskip_check_setting(d, states, B, "ctcd_stream_decode_to_host"))) return rc;
  if (!d->sk_on)
    return stream_decode_to_host_impl(d, states, is_eos, probs, seq_lens_host, B, T, V, beam, num_processes, cutoff_prob, cutoff_top_n, blank_id, log_input,
                                      alloc, alloc_user, out_sc, out_len, n_results, out_T, out_R, out_L, stream_, nullptr);
  // the filter is on.  Compact records hold 16-bit frame numbers, and a filtered stream reports indices among the frames it has SEEN:
  // this route is taken only while they fit (stream_blank_skip.h compact_route_ok); beyond, the stream ends through ctcd_stream_decode
  if (states[0]->scorer && states[0]->scorer->cbl) return fail(CTCD_EUNSUPPORTED, "a callback scorer's streams end through ctcd_stream_decode");
  for (int b = 0; b < B; ++b)
    if (!ctcsskip::compact_route_ok(states[b]->seen, T))
      return fail(CTCD_EUNSUPPORTED, "compact results hold 16-bit frame numbers: a filtered stream that has seen more than 65536 frames ends through ctcd_stream_decode");
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  std::lock_guard<std::mutex> sk_lock(d->mu_skip);
  SkChunk ck;
  if ((rc = sskip_front(d, states, probs, seq_lens_host, B, T, V, blank_id, log_input, stream, ck))) return rc;
  ctcsskip::StreamRemapItem *h_tab = nullptr;
  const ctcsskip::StreamRemapItem *d_tab = nullptr;
  if ((rc = sskip_remap_table(d, B, &h_tab, &d_tab))) return rc;
  for (int b = 0; b < B; ++b)  // (the frames a stream will have decoded when the remap runs: the guard)
    h_tab[b] = ctcsskip::StreamRemapItem{states[b]->map, nullptr, (int32_t)(states[b]->frames + ck.kept[b]), 0};
  return stream_decode_to_host_impl(d, states, is_eos, ck.rows, ck.kept.data(), B, T, V, beam, num_processes, cutoff_prob, cutoff_top_n, blank_id, ck.log_input,
                                    alloc, alloc_user, out_sc, out_len, n_results, out_T, out_R, out_L, stream_, d_tab, [&] { sskip_advance(d, states, B, ck); },
                                    ck.dtype);
}

static int stream_decode_to_host_impl(ctcd_decoder *d, ctcd_stream **states, const unsigned char *is_eos, const float *probs,
                                      const int32_t *seq_lens_host, int B, int T, int V, int beam, int num_processes, double cutoff_prob,
                                      int cutoff_top_n, int blank_id, int log_input, ctcd_result_alloc_fn alloc, void *alloc_user,
                                      float *out_sc, int32_t *out_len, int32_t *n_results, int out_T, int *out_R, int *out_L, void *stream_,
                                      const ctcsskip::StreamRemapItem *remap_tab, const std::function<void()> &launched, int in_dtype) {
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  if (states[0] && states[0]->scorer && states[0]->scorer->cbl) return fail(CTCD_EUNSUPPORTED, "a callback scorer's streams end through ctcd_stream_decode");
  if (out_T > 65536 || V > 65535) return fail(CTCD_EUNSUPPORTED, "compact results pack label and frame into 16 bits each");
  std::lock_guard<std::mutex> host_lock(d->mu_host);
  static const bool trace = getenv("CTCD_STREAM_TIMING") != nullptr;  // (stderr: where the call's time goes)
  const auto t0 = std::chrono::steady_clock::now();
  auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  double t_launch = 0, t_sync = 0, t_alloc = 0;
  std::vector<int32_t> lens(B);
  bool any_eos = false;
  int rc = stream_prepare(d, states, is_eos, seq_lens_host, B, T, V, beam, out_T, stream, lens, any_eos);
  if (rc) return rc;
  const size_t kk = (size_t)B * beam;
  const long long cap = std::max<long long>(ctcd_compact_label_capacity(B, beam, out_T), 1);
  if (cap > 0xFFFFFFFFLL) return fail(CTCD_EUNSUPPORTED, "batch too large for one compact label buffer; split the batch");
  if ((rc = d->c_hdr.ensure((size_t)B * 16)) || (rc = d->c_ent.ensure(kk * 16)) || (rc = d->c_rag.ensure((size_t)cap * 4)) ||
      (rc = d->c_cnt.ensure(256)) || (rc = d->c_sc.ensure(kk * 4)) || (rc = d->c_ln.ensure(kk * 4 + (size_t)B * 4)))
    return rc;
  int32_t *d_nres = (int32_t *)((char *)d->c_ln.p + kk * 4);
  // the page-locked mirror the kernel writes a finished stream's records to (as in ctcd_beam_decode_to_host)
  const size_t o_done = 256, o_hdr = (o_done + (size_t)B * 4 + 255) / 256 * 256, o_ent = o_hdr + (size_t)B * 16,
               o_lab = (o_ent + kk * 16 + 255) / 256 * 256;
  const size_t mcap = d->mirror_cap_override >= 0 ? (size_t)d->mirror_cap_override + 1 : std::max<size_t>((size_t)1 << 20, (size_t)cap / 3);
  const size_t need = o_lab + mcap * 4;
  if (d->h_stage_cap < need) {
    if (d->h_stage) (void)hipHostFree(d->h_stage);
    d->h_stage = nullptr;
    d->h_stage_cap = 0;
    HIP_TRY(hipHostMalloc(&d->h_stage, need, hipHostMallocMapped | hipHostMallocCoherent));
    d->h_stage_cap = need;
  }
  char *hs = (char *)d->h_stage, *ds = nullptr;
  HIP_TRY(hipHostGetDevicePointer((void **)&ds, d->h_stage, 0));
  volatile int32_t *done = (volatile int32_t *)(hs + o_done);
  for (int b = 0; b < B; ++b) done[b] = 0;
  std::memset(hs + o_hdr, 0, (size_t)B * 16);  // (streams that do not end write nothing)
  CompactOut co{(int32_t *)d->c_hdr.p, (int32_t *)d->c_ent.p, (uint32_t *)d->c_rag.p, (unsigned *)d->c_cnt.p, (unsigned)cap};
  if (!remap_tab) {  // (filtered streams: the records are remapped on the device first, and fetched from its buffers below)
    co.m_hdr = (int32_t *)(ds + o_hdr); co.m_ent = (int32_t *)(ds + o_ent); co.m_done = (int32_t *)(ds + o_done);
    co.m_rag = (uint32_t *)(ds + o_lab); co.m_cap = (unsigned)std::min<size_t>(mcap, 0xFFFFFFFFu);
  }
  StreamCall sc{states, is_eos, out_T, lens.data(), any_eos};
  sc.in_dtype = in_dtype;
  rc = decode_common(d, probs, nullptr, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, nullptr, nullptr, (float *)d->c_sc.p,
                     (int32_t *)d->c_ln.p, d_nres, stream, &sc, states[0]->scorer, &co);
  if (rc) return rc;
  for (int b = 0; b < B; ++b) states[b]->frames += lens[b];
  if (launched) launched();
  if (remap_tab && any_eos) {  // the frame half of every record goes back through the streams' maps (stream_blank_skip.h)
    if (d->timing) {
      if ((rc = sskip_timing_events(d))) return rc;
      HIP_TRY(hipEventRecord(d->ev_sk[2], stream));
    }
    const int e = ctcsskip::launch_remap_compact((const int32_t *)d->c_hdr.p, (const int32_t *)d->c_ent.p, (uint32_t *)d->c_rag.p, remap_tab, B, beam, (void *)stream);
    if (e != (int)hipSuccess) return fail(CTCD_EHIP, std::string("ctc_stream_remap_compact_kernel: ") + hipGetErrorString((hipError_t)e));
    if (d->timing) {
      HIP_TRY(hipEventRecord(d->ev_sk[3], stream));
      d->sk_remap_timed = true;
    }
    if ((rc = sskip_table_used(d, stream))) return rc;
  }
  struct Drain {
    hipStream_t a;
    ~Drain() { (void)hipStreamSynchronize(a); }
  } drain{stream};
  if (any_eos) {
    HIP_TRY(hipMemcpyAsync(out_sc, d->c_sc.p, kk * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out_len, d->c_ln.p, kk * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(n_results, d_nres, (size_t)B * 4, hipMemcpyDeviceToHost, stream));
  } else {
    std::memset(out_sc, 0, kk * 4); std::memset(out_len, 0, kk * 4); std::memset(n_results, 0, (size_t)B * 4);
  }
  t_launch = since();
  HIP_TRY(hipStreamSynchronize(stream));
  if ((rc = ctcd_check_status(d, B))) return rc;
  t_sync = since();
  if (!any_eos) return CTCD_OK;
  // the records: from the mirror, or -- an item whose labels fell beyond it -- everything from the device buffers
  const int32_t *hh = (const int32_t *)(hs + o_hdr), *he = (const int32_t *)(hs + o_ent);
  const uint32_t *hl = (const uint32_t *)(hs + o_lab);
  std::vector<int32_t> fh, fe;
  std::vector<uint32_t> fl;
  bool late = false;
  for (int b = 0; b < B; ++b) late |= is_eos[b] && done[b] != 1;
  if (late) {
    unsigned nlab = 0;
    HIP_TRY(hipMemcpy(&nlab, d->c_cnt.p, 4, hipMemcpyDeviceToHost));
    fh.resize((size_t)B * 4); fe.resize(kk * 4); fl.resize(nlab ? nlab : 1);
    HIP_TRY(hipMemcpy(fh.data(), d->c_hdr.p, (size_t)B * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fe.data(), d->c_ent.p, kk * 16, hipMemcpyDeviceToHost));
    if (nlab) HIP_TRY(hipMemcpy(fl.data(), d->c_rag.p, (size_t)nlab * 4, hipMemcpyDeviceToHost));
    hh = fh.data(); he = fe.data(); hl = fl.data();
  }
  int R = 0, L = 0;
  for (int b = 0; b < B; ++b) {
    const int nres = hh[(size_t)b * 4];
    R = std::max(R, nres);
    for (int j = 0; j < nres; ++j) L = std::max(L, he[((size_t)b * beam + j) * 4 + 2]);
  }
  if (out_R) *out_R = R;
  if (out_L) *out_L = L;
  int32_t *out_tok = nullptr, *out_ts = nullptr;
  if (alloc(alloc_user, R, L, &out_tok, &out_ts) != 0) return fail(CTCD_EINVAL, "the result allocator failed");
  t_alloc = since();
  if (R == 0 || L == 0) return CTCD_OK;
  if (!out_tok || !out_ts) return fail(CTCD_EINVAL, "the result allocator returned no buffers");
  if (!d->workers) d->workers = new HostPool;
  {
    const long long out_mb = (long long)B * R * L * 8 >> 20;
    const int want = std::max<long long>(num_processes, std::min<long long>(160, std::max<long long>(16, out_mb)));
    const int target = std::max(1, std::min(want, (int)std::thread::hardware_concurrency()));
    if (target > (int)d->workers->th.size()) d->workers->start(target - (int)d->workers->th.size());
  }
  d->workers->run(B, [=](int b) { ctcbeam::expand_item_host(hh, he, hl, b, beam, L, out_tok, out_ts, R); });
  if (trace) fprintf(stderr, "ctcd_stream_decode_to_host: queued %.3f ms, kernel done %.3f, buffers (R=%d, L=%d) %.3f, expanded by %d threads %.3f\n", t_launch, t_sync, R, L,
                     t_alloc, (int)d->workers->th.size(), since());
  return CTCD_OK;
}

int ctcd_beam_decode_host(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                          int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                          int32_t *out_tok, int32_t *out_ts, float *out_sc, int32_t *out_len, int32_t *n_results) {
  return ctcd_beam_decode_lm_host(d, probs, seq_lens, B, T, V, beam, num_processes, cutoff_prob, cutoff_top_n, blank_id, log_input,
                                  nullptr, out_tok, out_ts, out_sc, out_len, n_results);
}

// ---- compact result delivery.  The K label sequences of an utterance overlap almost entirely (the beam
// is a trie): a decode that hands over, per beam entry, only the labels it does not share with its DFS predecessor moves
// ~40x fewer bytes than the padded [B, K, T] pair -- over PCIe for the reference's CPU-tensor contract, over xGMI for the
// multi-GPU gather.  Layout: beam_core.h OutRefs::c_*.
long long ctcd_compact_label_capacity(int B, int beam, int T) { return (long long)B * beam * T; }  // worst case: nothing shared

int ctcd_beam_decode_compact(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                             int /*num_processes*/, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                             ctcd_scorer *scorer, int32_t *c_hdr, int32_t *c_ent, uint32_t *c_labels, uint32_t *c_count,
                             long long label_capacity, float *out_sc, int32_t *out_len, int32_t *n_results, void *stream_) {
  if (!c_hdr || !c_ent || !c_labels || !c_count || label_capacity <= 0) return fail(CTCD_EINVAL, "compact buffers missing");
  CompactOut co{c_hdr, c_ent, c_labels, c_count, (unsigned)std::min<long long>(label_capacity, 0xFFFFFFFFLL)};
  // (round 5) a callback scorer: launch after launch like the padded form; an utterance hands its compact records over in the
  // launch it finishes in, the buffers and their bump allocator carry over from launch to launch
  if (scorer && scorer->cbl)
    return decode_lm_callback(d, probs, seq_lens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, scorer, nullptr, nullptr, out_sc, out_len,
                              n_results, stream_, &co);
  return decode_common(d, probs, seq_lens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, nullptr, nullptr, out_sc,
                       out_len, n_results, stream_, nullptr, scorer, &co);
}

int ctcd_expand_compact(ctcd_decoder *d, const int32_t *c_hdr, const int32_t *c_ent, const uint32_t *c_labels, int B, int beam, int T,
                        int32_t *out_tok, int32_t *out_ts, void *stream_) {
  if (!d || B < 0 || beam <= 0 || T < 0) return fail(CTCD_EINVAL, "bad arguments");
  if (B == 0 || T == 0) return CTCD_OK;
  if (!c_hdr || !c_ent || !c_labels || !out_tok || !out_ts) return fail(CTCD_EINVAL, "null tensor");
  CTC_ON_DEVICE(d->device);
  if (beam > kExpandMaxK) return fail(CTCD_EUNSUPPORTED, "device expansion of compact results: beam_width > 4096");
  const size_t esm = ((size_t)5 * beam + (beam + 31) / 32 + 4) * 4;
  if (esm + 1024 > (size_t)d->max_lds) return fail(CTCD_EUNSUPPORTED, "device expansion of compact results: the entry tables of this beam width exceed one workgroup's LDS");
  HIP_TRY(hipFuncSetAttribute((const void *)expand_compact_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)esm));  // (beam > ~3270 needs more than the default 64 KB)
  hipLaunchKernelGGL(expand_compact_kernel, dim3(B), dim3(beam >= 16 ? 1024 : 256), esm, (hipStream_t)stream_, c_hdr, c_ent, c_labels, beam, T,
                     out_tok, out_ts);
  HIP_TRY(hipGetLastError());
  return CTCD_OK;
}

// Rows 0 .. n-1 alone, device tensors in and out, nothing read back in between: the decode hands its results over in compact
// form into the decoder's own scratch and the n-best expansion (nbest.hip) follows on the same stream.  Where the compact form
// is not to be had (T > 65536, T == 0, a callback scorer, a beam the expansion's tables do not fit) the decode writes its padded
// tensors into scratch and rows [:, :n] are copied out of them: the same results.  The scratch belongs to the decoder's next
// call, which is ordered behind this one on `stream`.
int ctcd_beam_decode_nbest(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam, int /*num_processes*/,
                           double cutoff_prob, int cutoff_top_n, int blank_id, int log_input, ctcd_scorer *scorer, int n_best, int32_t *out_tok,
                           int32_t *out_ts, float *out_sc, int32_t *out_len, int32_t *n_results, void *stream_) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  int rc = check_args(B, T, V, beam, cutoff_top_n, blank_id, probs, out_tok, out_ts, out_sc, out_len);
  if (rc) return rc;
  if (n_best < 1 || n_best > beam) return fail(CTCD_EINVAL, "n_best must be an integer in [1, beam_width]");
  if (B == 0) return CTCD_OK;
  std::lock_guard<std::mutex> host_lock(d->mu_host);  // (the scratch is the host-tensor entry points')
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  const size_t kk = (size_t)B * beam;
  const bool hook = scorer && scorer->cbl;
  const long long cap = ctcd_compact_label_capacity(B, beam, T);
  const ctcnbest::NbestDecoderInfo inf{d->device, d->max_lds};
  if (T > 65536 || V > 65535 || T == 0 || hook || cap > 0xFFFFFFFFLL || !ctcnbest::nbest_expand_fits(inf, beam, n_best)) {
    const size_t rowb = (size_t)T * 4, kt = kk * rowb, nb = (size_t)n_best;
    const size_t o_ts = (kt + 15) / 16 * 16, o_sc = o_ts * 2, o_ln = o_sc + (kk * 4 + 15) / 16 * 16, o_nr = o_ln + (kk * 4 + 15) / 16 * 16;
    if ((rc = d->stage_out.ensure(o_nr + (size_t)B * 4 + 16))) return rc;
    char *dout = (char *)d->stage_out.p;
    int32_t *nr = n_results ? n_results : (int32_t *)(dout + o_nr);
    if (hook)
      rc = decode_lm_callback(d, probs, seq_lens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, scorer, (int32_t *)dout,
                              (int32_t *)(dout + o_ts), (float *)(dout + o_sc), (int32_t *)(dout + o_ln), nr, stream);
    else
      rc = decode_common(d, probs, seq_lens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, (int32_t *)dout, (int32_t *)(dout + o_ts),
                         (float *)(dout + o_sc), (int32_t *)(dout + o_ln), nr, stream, nullptr, scorer);
    if (rc) return rc;
    if (rowb) {
      HIP_TRY(hipMemcpy2DAsync(out_tok, nb * rowb, dout, (size_t)beam * rowb, nb * rowb, (size_t)B, hipMemcpyDeviceToDevice, stream));
      HIP_TRY(hipMemcpy2DAsync(out_ts, nb * rowb, dout + o_ts, (size_t)beam * rowb, nb * rowb, (size_t)B, hipMemcpyDeviceToDevice, stream));
    }
    HIP_TRY(hipMemcpy2DAsync(out_sc, nb * 4, dout + o_sc, (size_t)beam * 4, nb * 4, (size_t)B, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpy2DAsync(out_len, nb * 4, dout + o_ln, (size_t)beam * 4, nb * 4, (size_t)B, hipMemcpyDeviceToDevice, stream));
    return CTCD_OK;
  }
  if ((rc = d->c_hdr.ensure((size_t)B * 16)) || (rc = d->c_ent.ensure(kk * 16)) || (rc = d->c_rag.ensure((size_t)cap * 4)) ||
      (rc = d->c_cnt.ensure(256)) || (rc = d->c_sc.ensure(kk * 4)) || (rc = d->c_ln.ensure(kk * 4 + (size_t)B * 4)))
    return rc;
  int32_t *nr = n_results ? n_results : (int32_t *)((char *)d->c_ln.p + kk * 4);
  CompactOut co{(int32_t *)d->c_hdr.p, (int32_t *)d->c_ent.p, (uint32_t *)d->c_rag.p, (unsigned *)d->c_cnt.p, (unsigned)cap};
  rc = decode_common(d, probs, seq_lens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, nullptr, nullptr, (float *)d->c_sc.p,
                     (int32_t *)d->c_ln.p, nr, stream, nullptr, scorer, &co);
  if (rc) return rc;
  return ctcnbest::launch_nbest_expand(inf, co.hdr, co.ent, co.rag, (unsigned long long)cap, (const float *)d->c_sc.p, (const int32_t *)d->c_ln.p, B, beam, T,
                                       n_best, out_tok, out_ts, out_sc, out_len, (int32_t *)d->status.p, stream);
}

// The reference's call as its Python makes it (ctcdecode/__init__.py:77-123 -> paddle_beam_decode[_lm]): the four results
// arrive as HOST tensors. probs / seq_lens may live on either side (probs_on_device != 0: both are device pointers).
// The kernel hands its results over in compact form, they cross PCIe compact, and host threads expand them.
static int decode_to_host_locked(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int probs_on_device, int B, int T, int V,
                                 int beam, int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                                 ctcd_scorer *scorer, int32_t *out_tok, int32_t *out_ts, float *out_sc, int32_t *out_len,
                                 int32_t *n_results, void *stream_, int n_best);

// (n_best: 0 = every row, the [B, beam, ...] tensors; n in [1, beam] = rows 0 .. n-1 alone, [B, n, ...] tensors)
static int decode_to_host(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int probs_on_device, int B, int T, int V,
                          int beam, int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                          ctcd_scorer *scorer, int32_t *out_tok, int32_t *out_ts, float *out_sc, int32_t *out_len,
                          int32_t *n_results, void *stream_, int n_best) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  int rc = check_args(B, T, V, beam, cutoff_top_n, blank_id, probs, out_tok, out_ts, out_sc, out_len);
  if (rc) return rc;
  if (!probs_on_device && d->in_dtype != CTCD_DTYPE_F32) return fail(CTCD_EUNSUPPORTED, "half-precision input from host memory (cast it to float32)");
  if (B == 0) return CTCD_OK;
  std::lock_guard<std::mutex> host_lock(d->mu_host);
  rc = decode_to_host_locked(d, probs, seq_lens, probs_on_device, B, T, V, beam, num_processes, cutoff_prob, cutoff_top_n, blank_id, log_input,
                             scorer, out_tok, out_ts, out_sc, out_len, n_results, stream_, n_best);
  if (rc == CTCD_EINTERNAL && d->input_timed_out) {
    // The streamed rows did not reach the kernel in time (its row fetch gives up after about a second): on this system the
    // copy stream evidently does not run beside the kernel.  Decode again the plain way, and stay with it.
    d->input_timed_out = false;
    d->no_input_streaming = true;
    if (d->copy_stream) (void)hipStreamSynchronize(d->copy_stream);
    rc = decode_to_host_locked(d, probs, seq_lens, probs_on_device, B, T, V, beam, num_processes, cutoff_prob, cutoff_top_n, blank_id, log_input,
                               scorer, out_tok, out_ts, out_sc, out_len, n_results, stream_, n_best);
  }
  return rc;
}

int ctcd_beam_decode_to_host(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int probs_on_device, int B, int T, int V,
                             int beam, int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                             ctcd_scorer *scorer, int32_t *out_tok, int32_t *out_ts, float *out_sc, int32_t *out_len,
                             int32_t *n_results, void *stream_) {
  return decode_to_host(d, probs, seq_lens, probs_on_device, B, T, V, beam, num_processes, cutoff_prob, cutoff_top_n, blank_id, log_input, scorer, out_tok,
                        out_ts, out_sc, out_len, n_results, stream_, 0);
}

int ctcd_beam_decode_to_host_nbest(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int probs_on_device, int B, int T, int V,
                                   int beam, int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                                   ctcd_scorer *scorer, int n_best, int32_t *out_tok, int32_t *out_ts, float *out_sc, int32_t *out_len,
                                   int32_t *n_results, void *stream_) {
  if (beam > 0 && (n_best < 1 || n_best > beam)) return fail(CTCD_EINVAL, "n_best must be an integer in [1, beam_width]");
  return decode_to_host(d, probs, seq_lens, probs_on_device, B, T, V, beam, num_processes, cutoff_prob, cutoff_top_n, blank_id, log_input, scorer, out_tok,
                        out_ts, out_sc, out_len, n_results, stream_, n_best);
}

static int decode_to_host_locked(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int probs_on_device, int B, int T, int V,
                                 int beam, int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                                 ctcd_scorer *scorer, int32_t *out_tok, int32_t *out_ts, float *out_sc, int32_t *out_len,
                                 int32_t *n_results, void *stream_, int n_best) {
  int rc;
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  const size_t nin = (size_t)B * T * V * 4, kk = (size_t)B * beam;
  const float *dprobs = probs;
  const int32_t *dlens = seq_lens;
  // Streamed input: with log-probabilities in host memory and no vocabulary pruning the kernel is launched BEFORE its
  // input has crossed PCIe; the rows follow frame block by frame block on a second stream (the input is [B, T, V]: a
  // block is a strided copy), each block followed by an update of the "frames arrived" counter the kernel's row fetch
  // waits on (beam_core.h decode_utterance).  Hides the 0.5 ms the 30 MB of a configs[1] batch take.
  const bool pruned_in = used_cutoff_prob(cutoff_prob) < 1.0 || cutoff_top_n < V;
  // (V <= the workgroup size the launch will use -- decode_common: the caller's, or at least 512 -- so that the kernel
  //  prefetches its rows: ADVICE r3; rows that are not prefetched wait as well since round 4, this keeps the fast form)
  const bool stream_in = !probs_on_device && log_input == 1 && !pruned_in && T >= 128 && T <= 65536 && V <= (d->threads ? d->threads : 512) &&
                         nin >= ((size_t)1 << 20) && !d->no_input_streaming && !d->profile && !(scorer && scorer->cbl);
  int nblk = 0;
  int blk[10];
  const int *frames_ready = nullptr;
  if (stream_in) {
    const size_t off_rows = 256, off_sl = off_rows + (nin + 15) / 16 * 16, fg_need = off_sl + (size_t)B * 4 + 16;
    if (d->fg_in_cap < fg_need) {
      if (d->fg_in) (void)hipFree(d->fg_in);
      d->fg_in = nullptr; d->fg_in_cap = 0;
      HIP_TRY(hipExtMallocWithFlags(&d->fg_in, fg_need, hipDeviceMallocFinegrained));
      d->fg_in_cap = fg_need;
    }
    if (!d->copy_stream) {
      HIP_TRY(hipStreamCreateWithFlags(&d->copy_stream, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&d->ev_in, hipEventDisableTiming));
      HIP_TRY(hipHostMalloc((void **)&d->h_cnt, 256, hipHostMallocDefault));
    }
    char *fg = (char *)d->fg_in;
    HIP_TRY(hipMemsetAsync(fg, 0, 4, stream));  // no frame has arrived
    if (seq_lens) HIP_TRY(hipMemcpyAsync(fg + off_sl, seq_lens, (size_t)B * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(d->ev_in, stream));
    HIP_TRY(hipStreamWaitEvent(d->copy_stream, d->ev_in, 0));  // (the blocks must not overtake the reset)
    dprobs = (const float *)(fg + off_rows);
    dlens = seq_lens ? (const int32_t *)(fg + off_sl) : nullptr;
    frames_ready = (const int *)fg;
    // a small first block, so that the kernel starts at once; the rest in seven equal parts
    blk[0] = 0; blk[1] = 16; nblk = 1;
    for (int c = 1; c <= 7; ++c) blk[++nblk] = 16 + (int)((long long)(T - 16) * c / 7);
  } else if (!probs_on_device) {
    const size_t off_sl = (nin + 15) / 16 * 16;
    if ((rc = d->stage_in.ensure(off_sl + (size_t)B * 4 + 16))) return rc;
    char *din = (char *)d->stage_in.p;
    if (nin) HIP_TRY(hipMemcpyAsync(din, probs, nin, hipMemcpyHostToDevice, stream));
    if (seq_lens) HIP_TRY(hipMemcpyAsync(din + off_sl, seq_lens, (size_t)B * 4, hipMemcpyHostToDevice, stream));
    dprobs = (const float *)din;
    dlens = seq_lens ? (const int32_t *)(din + off_sl) : nullptr;
  }
  const bool hook = scorer && scorer->cbl;  // a callback scorer: launch after launch (cb_rounds) into the padded tensors
  if (T > 65536 || V > 65535 || T == 0 || hook) {  // outside the compact format's 16-bit fields: the padded tensors travel
    const size_t kt = kk * T * 4;
    const size_t o_ts = (kt + 15) / 16 * 16, o_sc = o_ts * 2, o_ln = o_sc + (kk * 4 + 15) / 16 * 16, o_nr = o_ln + (kk * 4 + 15) / 16 * 16;
    if ((rc = d->stage_out.ensure(o_nr + (size_t)B * 4 + 16))) return rc;
    char *dout = (char *)d->stage_out.p;
    if (hook)
      rc = decode_lm_callback(d, dprobs, dlens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, scorer, (int32_t *)dout,
                              (int32_t *)(dout + o_ts), (float *)(dout + o_sc), (int32_t *)(dout + o_ln), (int32_t *)(dout + o_nr), stream);
    else
      rc = decode_common(d, dprobs, dlens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, (int32_t *)dout, (int32_t *)(dout + o_ts),
                         (float *)(dout + o_sc), (int32_t *)(dout + o_ln), (int32_t *)(dout + o_nr), stream, nullptr, scorer);
    if (rc) return rc;
    if ((rc = ctcd_check_status(d, B))) return rc;
    if (n_best) {  // rows [:, :n] alone cross PCIe (the full decode defines them everywhere: zero outside the valid region)
      const size_t rowb = (size_t)T * 4, nb = (size_t)n_best;
      if (rowb) {
        HIP_TRY(hipMemcpy2D(out_tok, nb * rowb, dout, (size_t)beam * rowb, nb * rowb, (size_t)B, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy2D(out_ts, nb * rowb, dout + o_ts, (size_t)beam * rowb, nb * rowb, (size_t)B, hipMemcpyDeviceToHost));
      }
      HIP_TRY(hipMemcpy2D(out_sc, nb * 4, dout + o_sc, (size_t)beam * 4, nb * 4, (size_t)B, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy2D(out_len, nb * 4, dout + o_ln, (size_t)beam * 4, nb * 4, (size_t)B, hipMemcpyDeviceToHost));
      if (n_results) HIP_TRY(hipMemcpy(n_results, dout + o_nr, (size_t)B * 4, hipMemcpyDeviceToHost));
      return CTCD_OK;
    }
    if (kt) {
      HIP_TRY(hipMemcpy(out_tok, dout, kt, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(out_ts, dout + o_ts, kt, hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(out_sc, dout + o_sc, kk * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_len, dout + o_ln, kk * 4, hipMemcpyDeviceToHost));
    if (n_results) HIP_TRY(hipMemcpy(n_results, dout + o_nr, (size_t)B * 4, hipMemcpyDeviceToHost));
    return CTCD_OK;
  }
  const long long cap = ctcd_compact_label_capacity(B, beam, T);
  if (cap > 0xFFFFFFFFLL) return fail(CTCD_EUNSUPPORTED, "batch too large for one compact label buffer; split the batch");
  if ((rc = d->c_hdr.ensure((size_t)B * 16)) || (rc = d->c_ent.ensure(kk * 16)) || (rc = d->c_rag.ensure((size_t)cap * 4)) ||
      (rc = d->c_cnt.ensure(256)) || (rc = d->c_sc.ensure(kk * 4)) || (rc = d->c_ln.ensure(kk * 4 + (size_t)B * 4)))
    return rc;
  int32_t *d_nres = (int32_t *)((char *)d->c_ln.p + kk * 4);
  // Page-locked, device-visible staging the KERNEL writes to: [done flags | hdr | ent | labels].  A workgroup that has
  // finished its utterance copies the compact results there itself and raises the utterance's flag (beam_core.h
  // OutRefs::m_*): the results cross PCIe while the stragglers of the launch are still being decoded, and host threads
  // expand utterance after utterance as the flags come up -- when the kernel ends only its last utterances are left.
  const size_t o_done = 256, o_hdr = (o_done + (size_t)B * 4 + 255) / 256 * 256, o_ent = o_hdr + (size_t)B * 16,
               o_lab = (o_ent + kk * 16 + 255) / 256 * 256;
  // the mirror holds a third of the worst case (typical sharing: a tenth); an utterance whose labels fall beyond it is
  // fetched from the device buffer afterwards
  const size_t mcap = d->mirror_cap_override >= 0 ? (size_t)d->mirror_cap_override + 1 : std::max<size_t>((size_t)1 << 20, (size_t)cap / 3);
  const size_t need = o_lab + mcap * 4;
  if (d->h_stage_cap < need) {
    if (d->h_stage) (void)hipHostFree(d->h_stage);
    d->h_stage = nullptr;
    d->h_stage_cap = 0;
    HIP_TRY(hipHostMalloc(&d->h_stage, need, hipHostMallocMapped | hipHostMallocCoherent));
    d->h_stage_cap = need;
  }
  char *hs = (char *)d->h_stage, *ds = nullptr;
  HIP_TRY(hipHostGetDevicePointer((void **)&ds, d->h_stage, 0));
  volatile int32_t *done = (volatile int32_t *)(hs + o_done);
  for (int b = 0; b < B; ++b) done[b] = 0;
  CompactOut co{(int32_t *)d->c_hdr.p, (int32_t *)d->c_ent.p, (uint32_t *)d->c_rag.p, (unsigned *)d->c_cnt.p, (unsigned)cap};
  co.m_hdr = (int32_t *)(ds + o_hdr); co.m_ent = (int32_t *)(ds + o_ent); co.m_done = (int32_t *)(ds + o_done);
  co.m_rag = (uint32_t *)(ds + o_lab); co.m_cap = (unsigned)std::min<size_t>(mcap, 0xFFFFFFFFu);
  rc = decode_common(d, dprobs, dlens, B, T, V, beam, cutoff_prob, cutoff_top_n, blank_id, log_input, nullptr, nullptr, (float *)d->c_sc.p,
                     (int32_t *)d->c_ln.p, d_nres, stream, nullptr, scorer, &co, frames_ready);
  if (rc) return rc;
  // From here on work is queued that reads the caller's input and writes the caller's outputs: no way out of this
  // function -- error or not -- without both streams drained.
  struct Drain {
    hipStream_t a, b;
    ~Drain() { if (b) (void)hipStreamSynchronize(b); (void)hipStreamSynchronize(a); }
  } drain{stream, stream_in ? d->copy_stream : nullptr};
  if (stream_in) {  // the kernel is queued and waits for its rows: send them, frame block by frame block
    char *fg = (char *)d->fg_in;
    const size_t pitch = (size_t)T * V * 4;
    for (int c = 0; c < nblk; ++c) {
      const int f0 = blk[c], f1 = blk[c + 1];
      if (f1 <= f0) continue;
      HIP_TRY(hipMemcpy2DAsync(fg + 256 + (size_t)f0 * V * 4, pitch, (const char *)probs + (size_t)f0 * V * 4, pitch, (size_t)(f1 - f0) * V * 4, (size_t)B,
                               hipMemcpyHostToDevice, d->copy_stream));
      d->h_cnt[c] = f1;
      if (!d->stall_input_test) HIP_TRY(hipMemcpyAsync(fg, &d->h_cnt[c], 4, hipMemcpyHostToDevice, d->copy_stream));
    }
  }
  if (n_best) {  // columns [:n] of the decode's [B, beam] scores and lengths (zero beyond an item's results)
    HIP_TRY(hipMemcpy2DAsync(out_sc, (size_t)n_best * 4, d->c_sc.p, (size_t)beam * 4, (size_t)n_best * 4, (size_t)B, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpy2DAsync(out_len, (size_t)n_best * 4, d->c_ln.p, (size_t)beam * 4, (size_t)n_best * 4, (size_t)B, hipMemcpyDeviceToHost, stream));
  } else {
    HIP_TRY(hipMemcpyAsync(out_sc, d->c_sc.p, kk * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out_len, d->c_ln.p, kk * 4, hipMemcpyDeviceToHost, stream));
  }
  if (n_results) HIP_TRY(hipMemcpyAsync(n_results, d_nres, (size_t)B * 4, hipMemcpyDeviceToHost, stream));
  const int rows_out = n_best ? n_best : beam;  // result rows per item in the caller's tensors
  {
    if (!d->workers) d->workers = new HostPool;
    // host threads that expand the results (memory-bound work: 8 bytes written per label position of the padded tensors;
    // the reference's default num_processes = 4 was chosen for its CPU decode): one per 4 MB of output, between 16 and 64,
    // more if the caller asks, never more than the machine has.  The pool grows when a later call wants more.
    const long long out_mb = (long long)B * rows_out * T * 8 >> 20;
    const int want = std::max<long long>(num_processes, std::min<long long>(64, std::max<long long>(16, out_mb / 4)));
    const int target = std::max(1, std::min(want, (int)std::thread::hardware_concurrency()));
    if (target > (int)d->workers->th.size()) d->workers->start(target - (int)d->workers->th.size());
  }
  const int32_t *hh = (const int32_t *)(hs + o_hdr), *he = (const int32_t *)(hs + o_ent);
  const uint32_t *hl = (const uint32_t *)(hs + o_lab);
  std::atomic<int> finished{0}, sync_rc{0};
  std::mutex late_mu;
  std::vector<int> late;  // utterances the kernel did not mirror (labels beyond the mirror) -- or that never reported
  // n-best: the rows below n alone are expanded (nbest.h); a malformed record is reported, its rows come out zero
  std::vector<unsigned char> row_ok(n_best ? (size_t)B * n_best : 0);
  unsigned char *rok = row_ok.data();
  std::atomic<int> bad_item{-1};
  const unsigned long long mir_labels = co.m_cap, dev_labels = (unsigned long long)cap;
  const int dev = d->device;
  // job 0 waits for the stream (kernel + the small copies above) and tells the others; jobs 1 .. B expand utterance i - 1
  // as soon as its flag is up
  d->workers->run(B + 1, [&, hh, he, hl, done, dev, stream](int i) {
    if (i == 0) {
      (void)hipSetDevice(dev);
      if (hipStreamSynchronize(stream) != hipSuccess) sync_rc = 1;
      finished = 1;
      return;
    }
    const int b = i - 1;
    int v;
    for (int spin = 0; (v = done[b]) == 0 && !finished.load(std::memory_order_acquire); ++spin)
      if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
    if (v == 0) v = done[b];  // (the kernel has ended: whatever it wrote is visible)
    std::atomic_thread_fence(std::memory_order_acquire);
    if (v == 1 && n_best) {
      if (ctcnbest::expand_item_nbest_host(hh, he, hl, mir_labels, b, beam, T, n_best, out_tok, out_ts, rok + (size_t)b * n_best)) bad_item = b;
    } else if (v == 1) {
      ctcbeam::expand_item_host(hh, he, hl, b, beam, T, out_tok, out_ts);
    } else {
      std::lock_guard<std::mutex> g(late_mu);
      late.push_back(b);
    }
  });
  if (sync_rc) return fail(CTCD_EHIP, "hipStreamSynchronize failed");
  if (stream_in) HIP_TRY(hipStreamSynchronize(d->copy_stream));  // (long done: the kernel has consumed every row)
  if ((rc = ctcd_check_status(d, B))) return rc;
  if (!late.empty()) {  // rare: fetch the whole compact form from the device and expand the utterances left
    std::vector<int32_t> fh((size_t)B * 4), fe(kk * 4);
    unsigned nlab = 0;
    HIP_TRY(hipMemcpy(&nlab, d->c_cnt.p, 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> fl(nlab ? nlab : 1);
    HIP_TRY(hipMemcpy(fh.data(), d->c_hdr.p, (size_t)B * 16, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fe.data(), d->c_ent.p, kk * 16, hipMemcpyDeviceToHost));
    if (nlab) HIP_TRY(hipMemcpy(fl.data(), d->c_rag.p, (size_t)nlab * 4, hipMemcpyDeviceToHost));
    const int *lt = late.data();
    const int32_t *ph = fh.data(), *pe = fe.data();
    const uint32_t *pl = fl.data();
    const unsigned long long fetched = std::min<unsigned long long>(nlab, dev_labels);
    if (n_best)
      d->workers->run((int)late.size(), [=, &bad_item](int i) {
        if (ctcnbest::expand_item_nbest_host(ph, pe, pl, fetched, lt[i], beam, T, n_best, out_tok, out_ts, rok + (size_t)lt[i] * n_best)) bad_item = lt[i];
      });
    else
      d->workers->run((int)late.size(), [=](int i) { ctcbeam::expand_item_host(ph, pe, pl, lt[i], beam, T, out_tok, out_ts); });
  }
  if (n_best) {
    for (size_t i = 0; i < row_ok.size(); ++i)
      if (!row_ok[i]) { out_sc[i] = 0.0f; out_len[i] = 0; }
    if (bad_item >= 0) return fail(CTCD_EINTERNAL, "malformed compact record for item " + std::to_string(bad_item.load()));
  }
  return CTCD_OK;
}

// paddle_beam_decode_lm as the reference's Python calls it (binding.cpp:122-140): CPU tensors in, CPU tensors out.
// scorer == NULL decodes without a language model.
int ctcd_beam_decode_lm_host(ctcd_decoder *d, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                             int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                             ctcd_scorer *scorer, int32_t *out_tok, int32_t *out_ts, float *out_sc, int32_t *out_len,
                             int32_t *n_results) {
  return ctcd_beam_decode_to_host(d, probs, seq_lens, 0, B, T, V, beam, num_processes, cutoff_prob, cutoff_top_n, blank_id, log_input,
                                  scorer, out_tok, out_ts, out_sc, out_len, n_results, nullptr);
}

// The normalisation that log_input == 2 applies, on its own (device pointers; `out` may alias `logits`): float32
// log_softmax over the last axis with the summation order documented at log_softmax_rows_kernel.
int ctcd_log_softmax(ctcd_decoder *d, const float *logits, const int32_t *seq_lens, int B, int T, int V, float *out, void *stream_) {
  if (!d || !logits || !out || B < 0 || T < 0 || V < 1) return fail(CTCD_EINVAL, "bad arguments");
  if (B == 0 || T == 0) return CTCD_OK;
  CTC_ON_DEVICE(d->device);
  hipStream_t stream = (hipStream_t)stream_;
  int rc;
  {
    std::lock_guard<std::mutex> lock(d->mu);
    if ((rc = ensure_tables(d))) return rc;
  }
  if (d->in_dtype != CTCD_DTYPE_F32) {  // (half rows in place: the float32 rows written would overrun rows not read yet)
    const size_t n = (size_t)B * T * V;
    const uintptr_t x0 = (uintptr_t)logits, x1 = x0 + n * in_elem_bytes(d->in_dtype), y0 = (uintptr_t)out, y1 = y0 + n * 4;
    if (x0 < y1 && y0 < x1) return fail(CTCD_EINVAL, "half-precision logits: `out` must not overlap them (in-place is float32 only)");
  }
  d->last_in_dtype = d->in_dtype;
  std::fill(d->pre_fn, d->pre_fn + 4, nullptr);
  return launch_log_softmax(d, logits, out, (long long)B * T, seq_lens, T, V, stream, d->in_dtype);
}

// HIP-event timing of the decode kernel alone, on the stream it is launched on (bench.py's roofline figure).
int ctcd_set_timing(ctcd_decoder *d, int on) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  CTC_ON_DEVICE(d->device);
  if (on && !d->ev0) {
    HIP_TRY(hipEventCreate(&d->ev0));
    HIP_TRY(hipEventCreate(&d->ev1));
    HIP_TRY(hipEventCreate(&d->ev2));
    HIP_TRY(hipEventCreate(&d->ev3));
  }
  d->timing = on != 0;
  return CTCD_OK;
}

int ctcd_last_kernel_ms(ctcd_decoder *d, float *ms) {
  if (!d || !ms || !d->ev0) return fail(CTCD_EINVAL, "timing not enabled");
  HIP_TRY(hipEventSynchronize(d->ev1));
  HIP_TRY(hipEventElapsedTime(ms, d->ev0, d->ev1));
  return CTCD_OK;
}

// Duration of the vocabulary-prune kernel of the last decode (pruned configurations only; timing must be on).
int ctcd_last_prune_ms(ctcd_decoder *d, float *ms) {
  if (!d || !ms || !d->ev2 || !d->prune_timed) return fail(CTCD_EINVAL, "no timed prune pass");
  CTC_ON_DEVICE(d->device);
  HIP_TRY(hipEventSynchronize(d->ev3));
  HIP_TRY(hipEventElapsedTime(ms, d->ev2, d->ev3));
  return CTCD_OK;
}
// From the end of the fast prune pass to the start of the decode kernel: prune_resolve_kernel over the flagged frames (and the copy
// of their count behind it).
int ctcd_last_resolve_ms(ctcd_decoder *d, float *ms) {
  if (!d || !ms || !d->ev2 || !d->prune_timed) return fail(CTCD_EINVAL, "no timed prune pass");
  CTC_ON_DEVICE(d->device);
  HIP_TRY(hipEventSynchronize(d->ev0));
  HIP_TRY(hipEventElapsedTime(ms, d->ev3, d->ev0));
  return CTCD_OK;
}

// Phase profile (tools/phase_profile.py): run the instrumented build of the kernel and read its per-utterance timers
// (wall_clock64 ticks of a 100 MHz clock, accumulated per phase by thread 0 of each workgroup).
int ctcd_debug_set_profile(ctcd_decoder *d, int on) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  d->profile = on != 0;
  return CTCD_OK;
}

// Workspace layout: 1 (default) = small shapes use the kernel variant whose LDS arrays sit at compile-time addresses,
// 0 = always the run-time layout.  Results are identical; the switch exists so tests can run both variants.
int ctcd_debug_set_fixed_layout(ctcd_decoder *d, int on) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  d->no_fixed_layout = on == 0;
  return CTCD_OK;
}

// Flagged prune frames: 1 (default) = the std::sort replay keeps its arrays in LDS when the row fits, 0 = always in global
// memory (the path of rows beyond ~11 000 labels).  Results are identical; the switch exists for the tests.  (Until round 3
// "0" sent the flagged frames to the host toolchain; nothing goes there any more.)
int ctcd_debug_set_prune_resolve(ctcd_decoder *d, int on) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  d->resolve_in_global = on == 0;
  return CTCD_OK;
}

// Raw-logit input (log_input == 2): 1 (default) = long rows take the workgroup kernels (log_softmax_rows_wg_kernel; in front of a
// vocabulary prune the fused prune_logits_wg_kernel), 0 = always the one-wave log_softmax pass followed by the separate prune.
// Results are identical; the switch exists so tests can compare the two.
int ctcd_debug_set_fused_logits(ctcd_decoder *d, int on) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  d->no_fused_logits = on == 0;
  return CTCD_OK;
}

// The workgroup prune kernel: 1 (default) = the row stays in registers between the two looks at it, 0 = it is read twice (the form of
// rounds 2-5; vocabularies beyond 10 240 labels always).  Identical results; tests compare the two.
int ctcd_debug_set_prune_registers(ctcd_decoder *d, int on) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  d->no_prune_reg = on == 0;
  return CTCD_OK;
}

// Barrier timeline of batch item 0 (profiling build): call with out == NULL to arm frames [frame0, frame0 + nframes) of
// the following decodes, with out != NULL (int64 [16][ctcd_debug_timeline_cap()]) to fetch: per wave, the shader clock
// at arrival at / departure from each barrier, in program order.
int ctcd_debug_timeline_cap(void) { return kTimelineCap; }
int ctcd_debug_timeline(ctcd_decoder *d, int frame0, int nframes, long long *out) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  if (!out) { d->tl_f0 = frame0; d->tl_nf = nframes; d->tl_armed = nframes > 0; return CTCD_OK; }
  if (!d->tl.p) return fail(CTCD_EINVAL, "no timeline recorded");
  CTC_ON_DEVICE(d->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d->tl.p, (size_t)16 * kTimelineCap * 8, hipMemcpyDeviceToHost));
  return CTCD_OK;
}

// beam of batch item 0 after every frame (profiling build): out = int32 [T][1 + 4*beam]
int ctcd_debug_beam_dump(ctcd_decoder *d, int on, int *out, int T, int beam) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  d->dbg_on = on != 0;
  if (out && d->dbg.p) {
    CTC_ON_DEVICE(d->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d->dbg.p, (size_t)T * (1 + 4 * (size_t)beam) * 4, hipMemcpyDeviceToHost));
  }
  return CTCD_OK;
}

int ctcd_debug_get_profile(ctcd_decoder *d, long long *out, int B) {
  if (!d || !out || B <= 0 || !d->prof.p) return fail(CTCD_EINVAL, "no profile recorded");
  CTC_ON_DEVICE(d->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d->prof.p, (size_t)B * 16 * 8, hipMemcpyDeviceToHost));
  return CTCD_OK;
}

// Device expf/logf/log_sum_exp against the host C library over a range of float bit patterns (tests only):
// mode 0: expf_nonpos(x), 1: logf_normal(x), x = bits lo, lo+stride, ... <= hi;  mode 2: lse(x, y) on n pairs.
int ctcd_debug_math_check(ctcd_decoder *d, int mode, uint32_t lo, uint32_t hi, uint32_t stride, const float *xs,
                          const float *ys, long long n_pairs, long long *checked, long long *mismatches);

// Number of frames of the last ctcd_beam_decode whose vocabulary prune was resolved on the host: none, ever (kept for callers
// of earlier rounds; the host path is gone).
long long ctcd_last_prune_host_rows(ctcd_decoder *d) { return d ? 0 : -1; }
int ctcd_last_scorer_rounds(ctcd_decoder *d) { return d ? d->last_cb_rounds : -1; }
int ctcd_last_scorer_waits(ctcd_decoder *d) { return d ? d->last_cb_waits : -1; }
int ctcd_set_scorer_wait(ctcd_decoder *d, int on) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  d->no_hook_wait = on == 0;
  return CTCD_OK;
}
int ctcd_set_scorer_filter(ctcd_decoder *d, int on) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  d->no_lmq_filter = on == 0;
  return CTCD_OK;
}
int ctcd_last_scorer_pairs(ctcd_decoder *d, long long *queued, long long *distinct, long long *repeat_same_item) {
  if (!d) return fail(CTCD_EINVAL, "decoder == NULL");
  if (queued) *queued = d->last_pairs[0];
  if (distinct) *distinct = d->last_pairs[1];
  if (repeat_same_item) *repeat_same_item = d->last_pairs[2];
  return CTCD_OK;
}
// ... and the number the fast prune pass flagged (settled by the device's std::sort replay + exact cumulative chain).  The
// count arrives behind the call's kernels: asking for it waits for the launch stream.
long long ctcd_last_prune_flagged_rows(ctcd_decoder *d) {
  if (!d) return -1;
  if (d->flagged_pending) {
    DeviceGuard g(d->device);
    if (hipStreamSynchronize(d->last_stream) != hipSuccess) return -1;
    d->prune_flagged_rows = d->h_flagged ? (long long)*d->h_flagged : 0;
    d->flagged_pending = false;
  }
  return d->prune_flagged_rows;
}

// The vocabulary-prune pass's output of the last call, copied to host memory (test hook: lets a test compare prune variants
// directly): cnt[rows], labels / values [rows][stride] with stride = min(cutoff_top_n, V); entries at or beyond a frame's count
// are unspecified.  Waits for the launch stream.
int ctcd_debug_prune_rows(ctcd_decoder *d, long long rows, int stride, int32_t *cnt, int32_t *labels, float *values) {
  if (!d || rows < 0 || stride < 1 || !cnt || !labels || !values) return fail(CTCD_EINVAL, "bad arguments");
  std::lock_guard<std::mutex> lock(d->mu);
  CTC_ON_DEVICE(d->device);
  if (d->pr_cnt.cap < (size_t)rows * 4 || d->pr_ch.cap < (size_t)rows * stride * 4 || d->pr_lp.cap < (size_t)rows * stride * 4)
    return fail(CTCD_EINVAL, "the last call's prune pass did not produce that many frames");
  HIP_TRY(hipStreamSynchronize(d->last_stream));
  HIP_TRY(hipMemcpy(cnt, d->pr_cnt.p, (size_t)rows * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(labels, d->pr_ch.p, (size_t)rows * stride * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(values, d->pr_lp.p, (size_t)rows * stride * 4, hipMemcpyDeviceToHost));
  return CTCD_OK;
}

// The same words, fetched without blocking: the copy into `host_status` (B words, page-locked memory for a truly
// asynchronous copy) is enqueued on `stream` -- pass the stream the decode was launched on, before enqueuing anything else
// there -- and the caller waits for its own event; 0 = ST_OK for an item, anything else is a failure code.  A pipelined
// caller (the next batch's kernel already queued behind) inspects a batch's outcome this way without draining the stream.
int ctcd_fetch_status_async(ctcd_decoder *d, int B, int32_t *host_status, void *stream_) {
  if (!d || B < 0 || (B > 0 && !host_status)) return fail(CTCD_EINVAL, "bad arguments");
  if (B == 0) return CTCD_OK;
  CTC_ON_DEVICE(d->device);
  if (!d->status.p || d->status.cap < (size_t)B * 4) return fail(CTCD_EINVAL, "no decode of that many items has been launched");
  HIP_TRY(hipMemcpyAsync(host_status, d->status.p, (size_t)B * 4, hipMemcpyDeviceToHost, (hipStream_t)stream_));
  return CTCD_OK;
}

// Status words of the last ctcd_beam_decode on this decoder (device -> host); for callers of the async entry point.
int ctcd_check_status(ctcd_decoder *d, int B) {
  if (!d || B < 0) return fail(CTCD_EINVAL, "bad arguments");
  CTC_ON_DEVICE(d->device);
  if (d->peek_items > 0) {  // a queued ctcd_stream_peek: its own status words first (B counts the items of the last decode launch; 0: the peek alone)
    std::vector<int32_t> ps((size_t)d->peek_items);
    d->peek_items = 0;
    HIP_TRY(hipMemcpyAsync(ps.data(), d->peek_status.p, ps.size() * 4, hipMemcpyDeviceToHost, d->peek_stream));
    HIP_TRY(hipStreamSynchronize(d->peek_stream));
    for (size_t b = 0; b < ps.size(); ++b) {
      if (ps[b] == ctcpeek::PEEK_ROW_OVERFLOW) return fail(CTCD_EINVAL, "ctcd_stream_peek: a result row of item " + std::to_string(b) + " does not fit L_cap");
      if (ps[b] != ctcpeek::PEEK_OK) return fail(CTCD_EINTERNAL, "ctcd_stream_peek: status " + std::to_string(ps[b]) + " for item " + std::to_string(b));
    }
  }
  if (B == 0) return CTCD_OK;
  if (!d->status.p || d->status.cap < (size_t)B * 4) return fail(CTCD_EINVAL, "no decode of that many items has been launched");
  const bool with_shape = d->status.cap >= (size_t)B * 8 && d->status_items == B;
  std::vector<int32_t> st((size_t)B * (with_shape ? 2 : 1));
  // ordered after the kernel on the stream it was launched on (a null-stream copy would not wait for a non-blocking stream)
  HIP_TRY(hipMemcpyAsync(st.data(), d->status.p, st.size() * 4, hipMemcpyDeviceToHost, d->last_stream));
  HIP_TRY(hipStreamSynchronize(d->last_stream));
  if (with_shape) {
    // The beam shape the launch ended with: entries of an item's final beam that have descendants in it (x 16), averaged over the
    // items.  Random rows: 1-2; blank-dominated rows: ~20.  The next launch's phase A1 is chosen by it (hysteresis 4 .. 8).
    long long sum = 0, cnt = 0;
    for (int b = 0; b < B; ++b)
      if (st[B + b] > 0 || st[b] == ST_OK) { sum += st[B + b]; ++cnt; }
    if (cnt) {
      const double per_frame = (double)sum / (double)cnt / 16.0;
      if (per_frame >= 8.0) d->subtree_on = true;
      else if (per_frame <= 4.0) d->subtree_on = false;
    }
  }
  for (int b = 0; b < B; ++b)
    if (st[b] != ST_OK) {
      if (st[b] == ST_INPUT_TIMEOUT) d->input_timed_out = true;
      return fail(CTCD_EINTERNAL, "decoder status " + std::to_string(st[b]) + " for item " + std::to_string(b));
    }
  return CTCD_OK;
}

int ctcd_debug_math_check(ctcd_decoder *d, int mode, uint32_t lo, uint32_t hi, uint32_t stride, const float *xs,
                          const float *ys, long long n_pairs, long long *checked, long long *mismatches) {
  if (!d || !checked || !mismatches || stride == 0) return fail(CTCD_EINVAL, "bad arguments");
  CTC_ON_DEVICE(d->device);
  int rc;
  if ((rc = ensure_tables(d))) return rc;
  *checked = 0;
  *mismatches = 0;
  const size_t chunk = (size_t)1 << 24;
  Buf out, inx, iny;
  if (mode >= 3 && mode <= 6) {  // binary64 log (3: log(p), 4: log(p + FLT_MIN)) / exp (5) on float images, log_sum_exp<double> on pairs (6)
    if ((rc = out.ensure(chunk * 8))) return rc;
    std::vector<uint64_t> h64(chunk);
    auto same = [](double want, uint64_t got) { return (want != want && ctcmath::bits_to_f64(got) != ctcmath::bits_to_f64(got)) || ctcmath::f64_to_bits(want) == got; };
    auto ref_lse64 = [](double x, double y) {  // decoder_utils.h:47-54, T = double
      const double neg = -DBL_MAX;
      if (x <= neg) return y;
      if (y <= neg) return x;
      const double m = x > y ? x : y;
      return std::log(std::exp(x - m) + std::exp(y - m)) + m;
    };
    if (mode == 6) {
      if (!xs || !ys || n_pairs < 0) return fail(CTCD_EINVAL, "pairs missing");
      if ((rc = inx.ensure(chunk * 4)) || (rc = iny.ensure(chunk * 4))) return rc;
      for (long long off = 0; off < n_pairs; off += (long long)chunk) {
        const size_t cnt = (size_t)std::min<long long>((long long)chunk, n_pairs - off);
        HIP_TRY(hipMemcpy(inx.p, xs + off, cnt * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(iny.p, ys + off, cnt * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(debug_math64_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0, 6, 0u, 1u, (const float *)inx.p, (const float *)iny.p, (uint64_t *)out.p, cnt);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(h64.data(), out.p, cnt * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; ++i)
          if (!same(ref_lse64((double)xs[off + i], (double)ys[off + i]), h64[i])) ++*mismatches;
        *checked += (long long)cnt;
      }
      inx.release();
      iny.release();
    } else {
      for (uint64_t start = lo; start <= hi; start += (uint64_t)chunk * stride) {
        const uint64_t cnt64 = ((uint64_t)hi - start) / stride + 1;
        const size_t cnt = (size_t)std::min<uint64_t>(cnt64, chunk);
        hipLaunchKernelGGL(debug_math64_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0, mode, (uint32_t)start, stride, (const float *)nullptr,
                           (const float *)nullptr, (uint64_t *)out.p, cnt);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(h64.data(), out.p, cnt * 8, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < cnt; ++i) {
          const double x = (double)ctcmath::bits_to_f32((uint32_t)(start + i * stride));
          const double want = mode == 3 ? std::log(x) : mode == 4 ? std::log(x + (double)FLT_MIN) : std::exp(x);
          if (!same(want, h64[i])) ++*mismatches;
        }
        *checked += (long long)cnt;
      }
    }
    out.release();
    return CTCD_OK;
  }
  if ((rc = out.ensure(chunk * 4))) return rc;
  std::vector<float> host(chunk);
  auto ref_lse = [](float x, float y) {  // decoder_utils.h:47-54
    const float neg = -FLT_MAX;
    if (x <= neg) return y;
    if (y <= neg) return x;
    const float m = x > y ? x : y;
    return std::log(std::exp(x - m) + std::exp(y - m)) + m;
  };
  if (mode == 0 || mode == 1) {
    for (uint64_t start = lo; start <= hi; start += (uint64_t)chunk * stride) {
      const uint64_t cnt64 = ((uint64_t)hi - start) / stride + 1;
      const size_t cnt = (size_t)std::min<uint64_t>(cnt64, chunk);
      hipLaunchKernelGGL(debug_math_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0, mode, (uint32_t)start, stride,
                         (const float *)nullptr, (const float *)nullptr, (float *)out.p, cnt, (const uint64_t *)d->tables.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(host.data(), out.p, cnt * 4, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < cnt; ++i) {
        const float x = ctcmath::bits_to_f32((uint32_t)(start + i * stride));
        const float want = mode == 0 ? std::exp(x) : std::log(x);
        const bool same = ctcmath::f32_to_bits(want) == ctcmath::f32_to_bits(host[i]);
        // below -88 the restatement returns 0 where libm returns < 2^-126: indistinguishable inside log_sum_exp
        if (!same && !(mode == 0 && x < -88.0f && host[i] == 0.0f && 1.0f + want == 1.0f)) ++*mismatches;
      }
      *checked += (long long)cnt;
    }
  } else {
    if (!xs || !ys || n_pairs < 0) return fail(CTCD_EINVAL, "pairs missing");
    if ((rc = inx.ensure(chunk * 4)) || (rc = iny.ensure(chunk * 4))) return rc;
    for (long long off = 0; off < n_pairs; off += (long long)chunk) {
      const size_t cnt = (size_t)std::min<long long>((long long)chunk, n_pairs - off);
      HIP_TRY(hipMemcpy(inx.p, xs + off, cnt * 4, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(iny.p, ys + off, cnt * 4, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(debug_math_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, 0, 2, 0u, 1u, (const float *)inx.p,
                         (const float *)iny.p, (float *)out.p, cnt, (const uint64_t *)d->tables.p);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(host.data(), out.p, cnt * 4, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < cnt; ++i)
        if (ctcmath::f32_to_bits(ref_lse(xs[off + i], ys[off + i])) != ctcmath::f32_to_bits(host[i])) ++*mismatches;
      *checked += (long long)cnt;
    }
    inx.release();
    iny.release();
  }
  out.release();
  return CTCD_OK;
}

}  // extern "C"
