// greedy_stream.hip -- greedy (best-path) CTC decoding of live streams (include/ctcdecode_amd.h "Greedy decode of live streams"): a
// stream fed chunk by chunk returns, call by call, the pieces of what ctcd_greedy_decode returns for all its frames together, bit for
// bit.  What a stream carries between calls is greedy.h's StreamRec, 32 bytes of device memory.  A chunk call queues, on the caller's
// stream and without a host read:
//   one copy of the call's per-stream arguments [record pointers | end-of-stream flags] (the decoder's page-locked staging)
//   greedy.hip's argmax pass on the chunk's [B, Tc, V] rows, as it stands
//   greedy_collapse_stream_kernel   a workgroup per stream, the layout of greedy_collapse_kernel (chunks of 1024 frames, a frame per
//                                   thread, ranks by ballot + popcount); what that kernel carries between its internal chunks -- the
//                                   label before the chunk, the open run's maximum, the score, the ranks -- comes from the record at
//                                   the start and goes back into it at the end
// Every store is a plain C++ store; there is no inline assembly.
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>
#include <vector>

#include "../../include/ctcdecode_amd.h"
#include "device_guard.h"
#include "greedy.h"
#include "lattice_device.h"

// One greedy stream: the device record and what the host knows without reading it.
struct ctcd_greedy_stream {
  int device = 0;
  ctcgreedy::StreamRec *rec = nullptr;  // device memory
  long long bound = 0;                  // F0 + the Tc of every call so far: an upper bound of F0 + the frames fed
  bool ended = false;
  unsigned long long seen_in_call = 0;  // "this stream is already part of the current call"
};

namespace ctcgreedy {

constexpr int kStreamThreads = 1024;  // frames of a collapse chunk = threads of the workgroup (16 waves)
constexpr int kStreamWaves = kStreamThreads / 64;

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// a record written on the stream (create, reset)
__global__ void greedy_stream_init_kernel(StreamRec *rec, int first_frame) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *rec = stream_rec_init(first_frame);
}

// One workgroup per stream of the call.  rec: the argmax pass's frame records, [B][T]; recs / eos: the staged arguments.  tokens /
// starts [B][T]; ends / label_scores [B][T + 1] and closed_lens [B], or NULL; scores / lens [B].  Ranks of this call start at 0; the run
// that came in open is closed entry 0 when greedy.h's carried_closes says so, and the ranks of the runs that end in the chunk follow it.
__global__ void __launch_bounds__(kStreamThreads) greedy_collapse_stream_kernel(const FrameRec *rec, const int32_t *seq_lens, int T, int blank,
                                                                               StreamRec *const *recs, const unsigned char *eos_flags, int32_t *tokens,
                                                                               int32_t *starts, int32_t *ends, float *label_scores, int32_t *closed_lens,
                                                                               float *scores, int32_t *lens) {
  __shared__ int s_lab[kStreamThreads];
  __shared__ float s_lp[kStreamThreads];
  __shared__ int s_cnt[2][kStreamWaves];  // a chunk's emit | run-end flags per wave
  __shared__ float s_open;                // the greatest lp so far of the run that is open at the chunk's end
  const int b = (int)blockIdx.x, tid = (int)threadIdx.x, wave = tid >> 6;
  const int n = ctcskip::clamped_len(seq_lens, b, T);
  const bool eos = eos_flags[b] != 0;
  StreamRec *const state = recs[b];
  const StreamRec R = *state;  // (every thread's copy; thread 0 writes the record behind the barriers below)
  const FrameRec *r = rec + (size_t)b * T;
  int32_t *tok = tokens + (size_t)b * T, *st = starts + (size_t)b * T, *en = ends ? ends + (size_t)b * (T + 1) : nullptr;
  float *ls = label_scores ? label_scores + (size_t)b * (T + 1) : nullptr;
  const bool carried = carried_closes(R, n, n > 0 ? r[0].c : blank, eos);
  int carry = 0;                    // labels emitted by the chunks so far
  int carry_end = carried ? 1 : 0;  // runs closed by the chunks so far
  float score = R.score;
  if (tid == 0) {
    s_open = R.open_max;
    if (carried) {
      if (en) en[0] = stream_frame_no(R, -1);
      if (ls) ls[0] = R.open_max;
    }
  }
  __syncthreads();
  for (int t0 = 0; t0 < n; t0 += kStreamThreads) {
    const int t = t0 + tid;
    const bool live = t < n;
    FrameRec me;
    me.c = blank;
    me.lp = 0.0f;
    if (live) me = r[t];
    const int before_chunk = t0 > 0 ? r[t0 - 1].c : rec_prev(R, blank);  // (the label of the frame before the chunk)
    const bool came_open = t0 > 0 || rec_open(R);                         // (a run of that label brings its maximum along in s_open)
    s_lab[tid] = me.c;
    s_lp[tid] = me.lp;
    __syncthreads();
    const int prev = tid > 0 ? s_lab[tid - 1] : before_chunk;
    int next = blank;
    if (t + 1 < n) next = tid + 1 < kStreamThreads ? s_lab[tid + 1] : r[t + 1].c;
    const bool emit = live && emits(me.c, prev, stream_first(R, t), blank), end = live && stream_run_ends(me.c, next, t, n, eos, blank);
    // the run goes on into the next chunk, or into the next call
    const bool open = live && !end && me.c != blank && (tid == kStreamThreads - 1 || stream_run_open(me.c, t, n, eos, blank));
    float rm = me.lp;
    if (end || open) {
      int k = tid;
      while (k > 0 && s_lab[k - 1] == me.c) {
        --k;
        rm = run_max_back(rm, s_lp[k]);
      }
      if (k == 0 && came_open && before_chunk == me.c) rm = run_max_back(rm, s_open);
    }
    const unsigned long long m_emit = __ballot(emit), m_end = __ballot(end);
    if ((tid & 63) == 0) {
      s_cnt[0][wave] = __popcll(m_emit);
      s_cnt[1][wave] = __popcll(m_end);
    }
    __syncthreads();
    int below = 0, total = 0, below_end = 0, total_end = 0;
#pragma unroll
    for (int w = 0; w < kStreamWaves; ++w) {
      const int ce = s_cnt[0][w], cx = s_cnt[1][w];
      below += w < wave ? ce : 0;
      total += ce;
      below_end += w < wave ? cx : 0;
      total_end += cx;
    }
    // (an emit rank is below the frames looked at so far: < n <= T; a run-end rank is at most one more: <= n < T + 1)
    if (emit) {
      const int i = carry + below + lanes_below(m_emit);
      tok[i] = me.c;
      st[i] = stream_frame_no(R, t);
    }
    if (end) {
      const int i = carry_end + below_end + lanes_below(m_end);
      if (en) en[i] = stream_frame_no(R, t);
      if (ls) ls[i] = rm;
    }
    if (open) s_open = rm;
    carry += total;
    carry_end += total_end;
    if (tid == 0) {
      const int cnt = n - t0 < kStreamThreads ? n - t0 : kStreamThreads;
#pragma unroll 8
      for (int k = 0; k < cnt; ++k) score = score_step(score, s_lp[k], stream_first(R, t0 + k));
    }
    __syncthreads();  // (s_lab, s_lp, s_cnt and s_open are reused by the next chunk; thread 0 reads s_open below)
  }
  if (tid == 0) {
    lens[b] = carry;
    scores[b] = score;
    if (closed_lens) closed_lens[b] = carry_end;
    *state = stream_rec_after(R, n, n > 0 ? r[n - 1].c : blank, carry, carry_end, score, s_open, eos, blank);
  }
  using ctclattice::zero_words;
  zero_words(tok + carry, T - carry, tid, kStreamThreads);
  zero_words(st + carry, T - carry, tid, kStreamThreads);
  if (en) zero_words(en + carry_end, T + 1 - carry_end, tid, kStreamThreads);
  if (ls) zero_words(reinterpret_cast<int32_t *>(ls) + carry_end, T + 1 - carry_end, tid, kStreamThreads);
}

std::atomic<unsigned long long> g_stream_calls{0};

int first_frame_ok(long long first_frame, const std::string &f) {
  if (first_frame < 0 || first_frame > kStreamMaxFrame) return ctcalign::align_fail(CTCD_EINVAL, (f + "0 <= first_frame <= 2^31 - 1 required").c_str());
  return CTCD_OK;
}
int hip_fail(const std::string &what, hipError_t e) { return ctcalign::align_fail(CTCD_EHIP, (what + ": " + hipGetErrorString(e)).c_str()); }

}  // namespace ctcgreedy

using namespace ctcgreedy;
using ctcalign::align_fail;

extern "C" {

int ctcd_greedy_stream_create(ctcd_decoder *d, ctcd_greedy_stream **out, long long first_frame) {
  const std::string f = "ctcd_greedy_stream_create: ";
  if (!d || !out) return align_fail(CTCD_EINVAL, (f + "decoder == NULL or out == NULL").c_str());
  *out = nullptr;
  if (const int rc = first_frame_ok(first_frame, f)) return rc;
  ctcalign::AlignDecoderInfo inf;
  if (const int rc = ctcalign::align_decoder_info(d, &inf)) return rc;
  ctcdev::DeviceGuard guard;
  if (guard.enter(inf.device) != hipSuccess) return hip_fail("hipSetDevice", guard.err);
  ctcd_greedy_stream *st = new ctcd_greedy_stream();
  st->device = inf.device;
  st->bound = first_frame;
  hipError_t e = hipMalloc((void **)&st->rec, sizeof(StreamRec));
  if (e == hipSuccess) {
    // (the record is in place when the call returns: the stream's first chunk may be queued on any stream)
    const StreamRec r = stream_rec_init((int)first_frame);
    e = hipMemcpy(st->rec, &r, sizeof r, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    if (st->rec) (void)hipFree(st->rec);
    delete st;
    return hip_fail(f + "the stream's record", e);
  }
  *out = st;
  return CTCD_OK;
}

void ctcd_greedy_stream_destroy(ctcd_decoder *d, ctcd_greedy_stream *st) {
  (void)d;
  if (!st) return;
  ctcdev::DeviceGuard guard;
  if (guard.enter(st->device) == hipSuccess && st->rec) (void)hipFree(st->rec);
  delete st;
}

int ctcd_greedy_stream_reset(ctcd_decoder *d, ctcd_greedy_stream *st, long long first_frame, void *stream) {
  const std::string f = "ctcd_greedy_stream_reset: ";
  if (!d || !st) return align_fail(CTCD_EINVAL, (f + "decoder == NULL or stream state == NULL").c_str());
  if (const int rc = first_frame_ok(first_frame, f)) return rc;
  ctcdev::DeviceGuard guard;
  if (guard.enter(st->device) != hipSuccess) return hip_fail("hipSetDevice", guard.err);
  hipLaunchKernelGGL(greedy_stream_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, st->rec, (int)first_frame);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(f + "the stream's record", e);
  st->bound = first_frame;
  st->ended = false;
  return CTCD_OK;
}

int ctcd_greedy_stream_decode(ctcd_decoder *d, ctcd_greedy_stream **states, const unsigned char *is_eos, const void *probs, const int32_t *seq_lens, int B, int Tc,
                              int V, int blank_id, int log_input, int32_t *out_tokens, int32_t *out_starts, int32_t *out_ends, float *out_label_scores,
                              int32_t *out_closed_lens, float *out_scores, int32_t *out_lens, void *stream) {
  const std::string f = "ctcd_greedy_stream_decode: ";
  if (!d) return align_fail(CTCD_EINVAL, "decoder == NULL");
  if (B < 0 || Tc < 0 || V < 1) return align_fail(CTCD_EINVAL, (f + "B, Tc >= 0 and V >= 1 required").c_str());
  if (blank_id < 0 || blank_id >= V) return align_fail(CTCD_EINVAL, "blank_id must index the vocabulary");
  if (log_input < 0 || log_input > 2) return align_fail(CTCD_EINVAL, (f + "log_input must be 0, 1 or 2").c_str());
  if (B == 0) return CTCD_OK;
  if (!states || !is_eos || !out_scores || !out_lens || (Tc > 0 && (!probs || !out_tokens || !out_starts)))
    return align_fail(CTCD_EINVAL, (f + "null tensor").c_str());
  if (V > (1 << 28)) return align_fail(CTCD_EUNSUPPORTED, (f + "V > 2^28").c_str());
  ctcalign::AlignDecoderInfo inf;
  if (const int rc = ctcalign::align_decoder_info(d, &inf)) return rc;
  const unsigned long long call = ++g_stream_calls;
  for (int b = 0; b < B; ++b) {
    ctcd_greedy_stream *st = states[b];
    if (!st) return align_fail(CTCD_EINVAL, (f + "a stream state is NULL").c_str());
    if (st->device != inf.device) return align_fail(CTCD_EINVAL, (f + "a stream state lives on another device than the decoder").c_str());
    if (st->ended) return align_fail(CTCD_EINVAL, (f + "a stream has ended: reset it before it is fed again").c_str());
    if (st->seen_in_call == call) return align_fail(CTCD_EINVAL, (f + "the same stream twice in one call").c_str());
    st->seen_in_call = call;
  }
  for (int b = 0; b < B; ++b)
    if (states[b]->bound + Tc > kStreamMaxFrame) return align_fail(CTCD_EUNSUPPORTED, (f + "a stream's frame numbers would pass 2^31 - 1").c_str());
  ctcdev::DeviceGuard guard;
  if (guard.enter(inf.device) != hipSuccess) return hip_fail("hipSetDevice", guard.err);
  hipStream_t s = (hipStream_t)stream;
  // [record pointers | end-of-stream flags]: one staged copy
  const size_t off_eos = (size_t)B * sizeof(StreamRec *);
  std::vector<unsigned char> args(off_eos + (size_t)B);
  for (int b = 0; b < B; ++b) {
    reinterpret_cast<StreamRec **>(args.data())[b] = states[b]->rec;
    args[off_eos + (size_t)b] = is_eos[b] ? 1 : 0;
  }
  void *dargs = nullptr, *rec = nullptr;
  if (Tc > 0)
    if (const int rc = greedy_scratch(d, greedy_scratch_bytes(B, Tc), &rec)) return rc;
  if (const int rc = greedy_stream_upload(d, args.data(), args.size(), stream, &dargs)) return rc;
  if (Tc > 0) {
    launch_argmax_pass(inf.in_dtype, log_input, probs, seq_lens, (long long)B * Tc, Tc, V, (FrameRec *)rec, stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("greedy argmax", e);
  }
  hipLaunchKernelGGL(greedy_collapse_stream_kernel, dim3((unsigned)B), dim3(kStreamThreads), 0, s, (const FrameRec *)rec, seq_lens, Tc, blank_id,
                     (StreamRec *const *)dargs, (const unsigned char *)dargs + off_eos, out_tokens, out_starts, out_ends, out_label_scores, out_closed_lens,
                     out_scores, out_lens);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("greedy stream collapse", e);
  for (int b = 0; b < B; ++b) {
    states[b]->bound += Tc;
    if (is_eos[b]) states[b]->ended = true;
  }
  return CTCD_OK;
}

int ctcd_greedy_stream_info(ctcd_decoder *d, const ctcd_greedy_stream *st, long long out[4]) {
  const std::string f = "ctcd_greedy_stream_info: ";
  if (!d || !st || !out) return align_fail(CTCD_EINVAL, (f + "decoder, stream state and out required").c_str());
  ctcdev::DeviceGuard guard;
  if (guard.enter(st->device) != hipSuccess) return hip_fail("hipSetDevice", guard.err);
  hipError_t e = hipDeviceSynchronize();  // (whatever stream the stream's calls were queued on)
  StreamRec r;
  if (e == hipSuccess) e = hipMemcpy(&r, st->rec, sizeof r, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(f + "the stream's record", e);
  out[0] = r.frames;
  out[1] = r.emitted;
  out[2] = r.closed;
  out[3] = rec_open(r) ? 1 : 0;
  return CTCD_OK;
}

}  // extern "C"
