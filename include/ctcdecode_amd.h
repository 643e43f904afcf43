/* ctcdecode_amd.h -- C ABI of the MI355X-native CTC prefix beam-search decoder.
 *
 * Drop-in boundary for the ONE hot path of parlance/ctcdecode: CTCBeamDecoder.decode() without a language model.
 * Each entry point names the reference interface it replaces (paths relative to the reference checkout):
 *
 *   ctcd_beam_decode        <- ctcdecode/src/binding.cpp:103-120  paddle_beam_decode()  (pybind11: binding.cpp:291)
 *                              = binding.cpp:35-101 beam_decode() -> ctc_beam_search_decoder_batch()
 *                                (ctcdecode/src/ctc_beam_search_decoder.cpp:245-285) with ext_scorer == nullptr
 *   ctcd_beam_decode_host   <- the same call as the reference makes it: CPU tensors in, CPU tensors out
 *                              (ctcdecode/__init__.py:77-123 moves probs to the CPU first; here they are staged to HBM)
 *   ctcd_create / destroy   <- no reference counterpart (the reference allocates per call); caches HBM scratch
 *   ctcd_last_error         <- replaces LOG(FATAL)/abort (ctcdecode/src/decoder_utils.h:17-29) by error codes
 *
 * Plain pointers and sizes only; no torch / HIP types.  `stream` is a hipStream_t passed as void* (NULL = default).
 * All functions return CTCD_OK (0) or a negative CTCD_E* code; ctcd_last_error() describes the last failure of the
 * calling thread.
 *
 * Tensor layouts (row-major, identical to the reference's tensors, ctcdecode/__init__.py:83-86):
 *   probs        float32 [B, T, V]   log_input == 1: log-probabilities; 0: probabilities (the reference's two modes,
 *                                    ctcdecode/__init__.py:42 log_probs_input); 2 (extension): raw logits, normalised on the
 *                                    device by a float32 log_softmax first (see ctcd_log_softmax)
 *   seq_lens     int32   [B] or NULL (all T); each clamped to [0, T]         (binding.cpp:64-65)
 *   out_tokens   int32   [B, beam, T] label ids   of beam p of item b at [b][p][0 .. out_lens[b][p])
 *   out_timesteps int32  [B, beam, T] frame index at which each label's probability peaked (path_trie.cpp:42-45)
 *   out_scores   float32 [B, beam]   negative log-likelihood, ascending = best first (decoder_utils.cpp:68)
 *   out_lens     int32   [B, beam]
 *   n_results    int32   [B] or NULL: number of beams actually returned for item b (min(beam, #prefixes))
 * Everything the reference leaves uninitialised (rows p >= n_results, positions >= out_lens) is written as 0.
 */
#ifndef CTCDECODE_AMD_H_
#define CTCDECODE_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTCD_OK 0
#define CTCD_EINVAL (-1)      /* bad argument (sizes, blank_id, NULL pointers, ...) */
#define CTCD_EUNSUPPORTED (-2) /* configuration outside what this build implements (see ctcd_last_error) */
#define CTCD_EHIP (-3)        /* HIP runtime error */
#define CTCD_EINTERNAL (-4)   /* decoder status word reported a failure */

typedef struct ctcd_decoder ctcd_decoder;

/* Create a decoder bound to HIP device `device_id`.  Owns only scratch (node pools, pruned candidate lists). */
int ctcd_create(ctcd_decoder **out, int device_id);
void ctcd_destroy(ctcd_decoder *dec);

/* Decode a batch whose tensors all live in the HBM of the decoder's device.  Asynchronous on `stream` -- call
 * hipStreamSynchronize (or ctcd_check_status / ctcd_fetch_status_async) before reading.  Nothing is read back or decided on
 * the host in between: the pre-passes (vocabulary pruning when cutoff_top_n < V or cutoff_prob < 1, with its std::sort replay
 * of the frames the fast pass flags; the probability -> log conversion when log_input == 0, binary64 log restated for the
 * device) and the decode kernel are queued behind each other on `stream`; see DESIGN.md 5. */
int ctcd_beam_decode(ctcd_decoder *dec, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                     int num_processes /* accepted for signature parity; unused on the GPU */, double cutoff_prob,
                     int cutoff_top_n, int blank_id, int log_input, int32_t *out_tokens, int32_t *out_timesteps,
                     float *out_scores, int32_t *out_lens, int32_t *n_results, void *stream);

/* log_softmax over the last axis of float32 [B, T, V] device memory, `out` may alias `logits` (no reference counterpart:
 * its callers run torch's log_softmax before decode(), README.md:30-38).  This is what log_input == 2 applies.  Defined
 * to the bit: y_j = (x_j - m) - logf(s), m = max x (NaNs skipped, a zero maximum taken as +0), s = sum_j expf(x_j - m) in float32 with lane l = j mod 64 adding its
 * terms in increasing j and the 64 partial sums combined by a butterfly (^1, ^2, ... ^32); expf / logf as in glibc, expf
 * below -88 taken as 0.  Frames at or beyond seq_lens[b] are not touched.  Asynchronous on `stream`. */
int ctcd_log_softmax(ctcd_decoder *dec, const float *logits, const int32_t *seq_lens, int B, int T, int V, float *out, void *stream);

/* Same, with HOST pointers for every tensor (what paddle_beam_decode receives).  Synchronous: when it returns -- with or
 * without an error -- nothing queued by the call still reads `probs` or writes the outputs.  Both PCIe legs overlap the
 * kernel: log-probability input without pruning is streamed to the already running kernel on a second
 * stream the decoder owns; finished utterances write their results into page-locked host memory themselves and host
 * threads (max(num_processes, 16)) expand them into the padded tensors.  `probs` may be pageable. */
int ctcd_beam_decode_host(ctcd_decoder *dec, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                          int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                          int32_t *out_tokens, int32_t *out_timesteps, float *out_scores, int32_t *out_lens,
                          int32_t *n_results);

/* ---- Compact result delivery (no reference counterpart: the reference fills two padded [B, beam, T] tensors,
 * binding.cpp:85-99).  The beam is a trie, so its label sequences overlap almost entirely; in compact form every beam
 * entry hands over only the labels it does not share with its predecessor in trie (DFS) order:
 *   c_hdr    int32 [B][4]        {#results, #labels of the item, index of its first label in c_labels, 0}
 *   c_ent    int32 [B][beam][4]  per entry j in DFS order: {result row, #labels shared with entry j-1, length, index of its own labels}
 *   c_labels uint32 [capacity]   label | frame << 16 (T <= 65536, V <= 65535), one bump-allocated buffer for the batch
 *   c_count  uint32 [1]          labels used (device word, zeroed by the call)
 * ctcd_beam_decode_compact = ctcd_beam_decode[_lm] (scorer may be NULL) writing this form (everything device memory);
 * ctcd_expand_compact rebuilds out_tokens / out_timesteps [B, beam, T] on the device (e.g. on the rank that gathered them);
 * ctcd_beam_decode_to_host is the reference's whole call -- results as HOST tensors, inputs on either side -- with the
 * compact form crossing PCIe and `num_processes` host threads expanding it. */
long long ctcd_compact_label_capacity(int B, int beam, int T);
typedef struct ctcd_scorer ctcd_scorer;
int ctcd_beam_decode_compact(ctcd_decoder *dec, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                             int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                             ctcd_scorer *scorer, int32_t *c_hdr, int32_t *c_ent, uint32_t *c_labels, uint32_t *c_count,
                             long long label_capacity, float *out_scores, int32_t *out_lens, int32_t *n_results, void *stream);
int ctcd_expand_compact(ctcd_decoder *dec, const int32_t *c_hdr, const int32_t *c_ent, const uint32_t *c_labels, int B, int beam,
                        int T, int32_t *out_tokens, int32_t *out_timesteps, void *stream);
int ctcd_beam_decode_to_host(ctcd_decoder *dec, const float *probs, const int32_t *seq_lens, int probs_on_device, int B, int T, int V,
                             int beam, int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                             ctcd_scorer *scorer, int32_t *out_tokens, int32_t *out_timesteps, float *out_scores,
                             int32_t *out_lens, int32_t *n_results, void *stream);

/* ---- LM tier: the external scorer.  Replaces ctcdecode/src/binding.cpp:122-150,263-287:
 *   ctcd_scorer_create          <- paddle_get_scorer(alpha, beta, lm_path, labels, vocab_size)   (binding.cpp:143-150)
 *   ctcd_scorer_destroy         <- paddle_release_scorer                                          (binding.cpp:263-265)
 *   ctcd_scorer_is_character_based / _max_order / _dict_size / _reset_params <- binding.cpp:271-287
 *   ctcd_beam_decode_lm[_host]  <- paddle_beam_decode_lm: paddle_beam_decode plus `void *scorer`  (binding.cpp:122-140)
 * The scorer object (ctcdecode/src/scorer.h:41-110) is built on the host from an ARPA text model (binary kenlm files are
 * not supported) and the label strings; its tables -- n-gram back-off automaton, dictionary trie -- are mirrored into the
 * HBM of `device_id` once, and the per-frame queries of DecoderState::next() run inside the decode kernel.  `labels`:
 * V NUL-terminated UTF-8 strings.  Word models need a " " label and at most 64 labels.  LM arithmetic follows kenlm's
 * published algorithm (float32 weights, longest listed n-gram, back-off weights added in float32); see DESIGN.md for
 * what this parity is pinned to. */
int ctcd_scorer_create(ctcd_scorer **out, double alpha, double beta, const char *lm_path, const char *const *labels, int V,
                       int device_id);
void ctcd_scorer_destroy(ctcd_scorer *scorer);
int ctcd_scorer_is_character_based(const ctcd_scorer *scorer);
int ctcd_scorer_max_order(const ctcd_scorer *scorer);
int ctcd_scorer_dict_size(const ctcd_scorer *scorer);
int ctcd_scorer_reset_params(ctcd_scorer *scorer, double alpha, double beta);
/* Scorer::get_log_cond_prob (scorer.cpp:74-93) on explicit words, evaluated on the host copy of the tables (tests). */
double ctcd_scorer_cond_log_prob(const ctcd_scorer *scorer, const char *const *words, int n);
/* ---- The swappable scorer: a scorer whose language model lives behind a HOST callback.  The reference's decoder takes an
 * opaque `void *scorer` (binding.cpp:122-140) and only ever calls Scorer::get_log_cond_prob(words) on the language-model side
 * (scorer.h:41-78, scorer.cpp:74-93; called from ctc_beam_search_decoder.cpp:120-137 with the window make_ngram built,
 * scorer.cpp:163-194); this is that interface across the C ABI, for models the built-in ARPA tables do not cover (binary
 * kenlm files through the `kenlm` module, a neural LM, a remote service ...).
 *   fn(user, words, n, &log10_prob): the window's n = max_order words, oldest first, "<s>"-padded as make_ngram pads them;
 *     store log10 p(words[n-1] | words[0..n-2]) as float32 -- what kenlm's BaseScore returns, the decoder applies the
 *     reference's conversion p / NUM_FLT_LOGE (scorer.cpp:92) -- and return 0; return 1 if the window holds a word the model
 *     does not know (the reference's OOV_SCORE, scorer.cpp:86-88); return < 0 to fail the decode.  The value must be
 *     finite (NaN or +-inf with return code 0 fails the decode: -inf is how the cache marks an OOV answer).  Must be a pure function
 *     of the words: answers are cached on the device ((history, word) -> log10 prob, the same tables the built-in scorer
 *     queries inside the kernel) and each distinct window is asked for once per scorer.  Called on the thread that calls
 *     the decode, between kernel launches: a launch runs until an utterance needs a window that is not cached, parks that
 *     utterance at the frame boundary, and resumes after the host has asked.
 *   vocabulary: the model's words (what Scorer::fill_dictionary reads from the model, scorer.cpp:196-230): builds the
 *     dictionary of a word model; all entries single characters <=> character model (scorer.cpp:65-71).
 *   Results equal those of a scorer that knew every answer from the start (tests/test_gpu_lm.py: the built-in tables behind
 *   the callback give bit-identical output).  Accepted by ctcd_beam_decode_lm, ctcd_beam_decode_lm_host,
 *   ctcd_beam_decode_to_host, ctcd_beam_decode_compact (since round 5: the compact multi-GPU gather works with it) and
 *   ctcd_stream_create_lm / ctcd_stream_decode.
 *   Since round 6 without shape restrictions: rows that hold +-inf or overflow float32 sums, and beams of any width the decoder
 *   takes (the wide-beam layouts), decode behind a callback as they do with the built-in tables.
 *   Decodes that share one callback scorer are serialised (its cache is one object) and the callback runs under that lock:
 *   a callback that itself decodes with the same scorer deadlocks.  A ctcd_stream_decode call that fails half-way (the
 *   callback reported an error) leaves the streams of that call unusable: destroy them.
 *   Cost: a warm cache decodes in one launch, like the built-in tables.  Cold, an utterance misses once per frame in which a
 *   prefix completes a word under a history it has not asked about; since round 6 its workgroup WAITS for the answer (see
 *   ctcd_last_scorer_waits below) instead of ending its launch, and the call is bound by the calling thread: the callback's own
 *   time plus ~0.12 us of bookkeeping per queued pair (bench.py "scorer hook": 128 x 1500 frames of transcript-like rows under a
 *   5-gram model, 195 k windows, 86-88 ms cold in one launch -- 264 ms and 699 launches in round 5).  ctcd_last_scorer_rounds tells
 *   how many launches the last call took.  The cache of such a scorer starts with room for 2 M windows (64 + 32 MB of HBM).
 * ctcd_scorer_cond_log10 evaluates any scorer in the callback's own form (so the built-in tables can sit behind one);
 * ctcd_scorer_callback_calls counts the windows the callback has answered so far (= distinct windows cached; for the batched form
 * below too). */
typedef int (*ctcd_cond_log10_fn)(void *user, const char *const *words, int n, float *log10_prob);
int ctcd_scorer_create_callback(ctcd_scorer **out, double alpha, double beta, int max_order, const char *const *vocabulary,
                                int n_vocabulary, ctcd_cond_log10_fn fn, void *user, const char *const *labels, int V, int device_id);
int ctcd_scorer_cond_log10(const ctcd_scorer *scorer, const char *const *words, int n, float *log10_prob);
long long ctcd_scorer_callback_calls(const ctcd_scorer *scorer);
/* seconds spent inside the callback so far (wall time of the asking passes of waiting launches; elsewhere every 16th call is timed
 * and counted sixteen times) */
double ctcd_scorer_callback_seconds(const ctcd_scorer *scorer);
/* A callback that may be called from several threads at once (a read-only model behind it; NOT a Python callable: the interpreter
 * lock serialises those): `threads` - 1 helper threads ask beside the calling thread while a launch waits for its answers -- the new
 * windows of a batch of queued pairs are split among them; caching the answers stays with the calling thread, so results and the
 * "every window is asked once" property are unchanged.  The helpers spin while a waiting launch is served and sleep otherwise.
 * 1 (the default): the callback is only ever called from the thread that called the decoder.  threads in [1, 64]. */
int ctcd_scorer_set_callback_threads(ctcd_scorer *scorer, int threads);
/* launches the decoder's last call through a callback scorer took (1 = the cache held everything; one more per round of
 * misses): what a cold / lukewarm cache costs (bench.py "scorer hook") */
int ctcd_last_scorer_rounds(ctcd_decoder *dec);
/* Since round 6 a launch WAITS for the callback's answers: a workgroup whose utterance misses stays on its CU, the calling thread
 * -- polling a miss list in page-locked memory -- asks the callback and publishes the answered cache slots, and the workgroup takes
 * the utterance up again; a relaunch remains for what cannot be done under a running kernel (the cache table or the state arrays
 * have to grow).  ctcd_last_scorer_waits: the answer batches the last call's launches were handed that way;
 * ctcd_set_scorer_wait(dec, 0): every miss ends the utterance's launch, as in rounds 4-5 (identical results; tests run both). */
int ctcd_last_scorer_waits(ctcd_decoder *dec);
int ctcd_set_scorer_wait(ctcd_decoder *dec, int on);

/* The batched form of the callback: one call asks many windows.
 *   fn(user, words, n_windows, order, log10_probs, status): words = n_windows * order pointers, window-major, each window oldest
 *     word first and "<s>"-padded exactly like ctcd_cond_log10_fn's; per window store log10_probs[i] and status[i] = 0 (ok) or
 *     1 (out of vocabulary; log10_probs[i] is ignored).  Return 0, or < 0 to fail the decode.  The contract is the per-window one:
 *     a pure function of the words, each distinct window asked once per scorer, NaN or +-inf with status 0 fails the decode, and
 *     it is called on the thread that called the decoder.
 *   Windows the device cache or the serving loop already answers never reach it.  The serving loop (the waiting launch and the
 *   launch-per-round path alike) reads the queued pairs in passes of at most 512 and asks the new windows of a pass in one call:
 *   a larger pass costs fewer calls but holds back the answers the first waiting workgroups need.  A batched scorer takes no
 *   helper threads (ctcd_scorer_set_callback_threads refuses threads > 1 with CTCD_EUNSUPPORTED).
 * ctcd_scorer_cond_log10_batch has the batched signature and evaluates any scorer (the batched counterpart of
 * ctcd_scorer_cond_log10: built-in tables behind the batched hook).  ctcd_scorer_callback_calls keeps counting WINDOWS;
 * ctcd_scorer_callback_batches counts calls of a batched callback (0 for the per-window form). */
typedef int (*ctcd_cond_log10_batch_fn)(void *user, const char *const *words, int n_windows, int order, float *log10_probs,
                                        int32_t *status);
int ctcd_scorer_create_callback_batch(ctcd_scorer **out, double alpha, double beta, int max_order, const char *const *vocabulary,
                                      int n_vocabulary, ctcd_cond_log10_batch_fn fn, void *user, const char *const *labels, int V,
                                      int device_id);
int ctcd_scorer_cond_log10_batch(const ctcd_scorer *scorer, const char *const *words, int n_windows, int order, float *log10_probs,
                                 int32_t *status);
long long ctcd_scorer_callback_batches(const ctcd_scorer *scorer);
/* Queued (history, word) pairs of the decoder's last call through a callback scorer: *queued = pairs the kernels queued and the
 * host read, *distinct = windows the call asked the callback for (its new cache entries), *repeat_same_item = queued pairs that
 * the item which first queued the pair in this call queued again.  A callback scorer's kernels drop repeated misses of one
 * utterance while it is parked (a small per-workgroup filter in LDS, cleared whenever the utterance is taken up);
 * ctcd_set_scorer_filter(dec, 0) turns that off (measurements, tests: identical results, more queued pairs). */
int ctcd_last_scorer_pairs(ctcd_decoder *dec, long long *queued, long long *distinct, long long *repeat_same_item);
int ctcd_set_scorer_filter(ctcd_decoder *dec, int on);

int ctcd_beam_decode_lm(ctcd_decoder *dec, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                        int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input, ctcd_scorer *scorer,
                        int32_t *out_tokens, int32_t *out_timesteps, float *out_scores, int32_t *out_lens, int32_t *n_results,
                        void *stream);
int ctcd_beam_decode_lm_host(ctcd_decoder *dec, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam,
                             int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                             ctcd_scorer *scorer, int32_t *out_tokens, int32_t *out_timesteps, float *out_scores,
                             int32_t *out_lens, int32_t *n_results);

/* ---- Streaming ("online") decoding: replaces ctcdecode/src/binding.cpp:153-265 (paddle_get_decoder_state,
 * paddle_beam_decode_with_given_state, paddle_release_state) = DecoderState objects kept alive between calls
 * (ctcdecode/src/ctc_beam_search_decoder.cpp:230-243,288-317).  A ctcd_stream parks one utterance's beam and node pool
 * in HBM between launches; frame numbers in `timesteps` keep counting across chunks (abs_time_step, :69).
 * ctcd_stream_decode feeds chunk b (probs[b, 0:min(seq_lens_host[b], T)], DEVICE pointer) to states[b]; where
 * is_eos[b] != 0 the stream's final beams are written to row b of the outputs (row stride out_T >= total frames of that
 * stream), elsewhere row b stays zero and n_results[b] = 0.  seq_lens_host and is_eos are HOST arrays (B entries). */
typedef struct ctcd_stream ctcd_stream;
int ctcd_stream_create(ctcd_decoder *dec, ctcd_stream **out, int V, int beam, int frames_hint);
/* paddle_get_decoder_state with a scorer (binding.cpp:243-261): the stream decodes with the LM tier */
int ctcd_stream_create_lm(ctcd_decoder *dec, ctcd_stream **out, int V, int beam, int frames_hint, ctcd_scorer *scorer);
void ctcd_stream_destroy(ctcd_decoder *dec, ctcd_stream *st);
long long ctcd_stream_frames(const ctcd_stream *st);
int ctcd_stream_decode(ctcd_decoder *dec, ctcd_stream **states, const unsigned char *is_eos, const float *probs,
                       const int32_t *seq_lens_host, int B, int T, int V, int beam, int num_processes, double cutoff_prob,
                       int cutoff_top_n, int blank_id, int log_input, int32_t *out_tokens, int32_t *out_timesteps,
                       float *out_scores, int32_t *out_lens, int32_t *n_results, int out_T, void *stream);

/* The same call with the results delivered to HOST memory in the reference's own sizes (binding.cpp:186-205 resizes its tensors
 * to [B, R, L]: R = the most results of any stream that ended, L = the longest of their label sequences).  R and L exist only
 * once the kernel has run, so the caller passes an allocator: it is called once, with (R, L), and returns the two int32 buffers
 * of B * R * L elements (return non-zero to fail the call; with R * L == 0 the buffers are not touched).  The finished streams'
 * results cross PCIe in compact form and host threads expand them (as ctcd_beam_decode_to_host does for the one-shot call).
 * `probs` is a DEVICE pointer; out_scores / out_lens [B, beam], n_results [B], *out_R, *out_L are HOST memory.  Synchronous.
 * Streams behind a callback scorer end through ctcd_stream_decode (CTCD_EUNSUPPORTED here). */
typedef int (*ctcd_result_alloc_fn)(void *user, int R, int L, int32_t **tokens, int32_t **timesteps);
int ctcd_stream_decode_to_host(ctcd_decoder *dec, ctcd_stream **states, const unsigned char *is_eos, const float *probs,
                               const int32_t *seq_lens_host, int B, int T, int V, int beam, int num_processes, double cutoff_prob,
                               int cutoff_top_n, int blank_id, int log_input, ctcd_result_alloc_fn alloc, void *alloc_user,
                               float *out_scores, int32_t *out_lens, int32_t *n_results, int out_T, int *out_R, int *out_L, void *stream);

/* Interim results of live streams (extension; the reference reports nothing before is_eos): what DecoderState::decode()
 * (ctc_beam_search_decoder.cpp:164-211, which does not change the state) would return now -- the result list of the one-shot decode
 * of the frames fed so far.  No frame is fed and nothing a later chunk reads is written.  Per stream b, with n = min(n_best, results):
 * n_results[b] = n; out_scores / out_lens [b, p] for p < n (the FULL length of row p); out_tokens / out_timesteps [b, p, q - since[b]]
 * for since[b] <= q < length (since_host == NULL: 0; a row shorter than since[b] reports no labels); stable_lens[b] = the length of
 * the longest common prefix of ALL current beam entries -- a prefix of every hypothesis the stream can still produce: it only grows,
 * and its labels and time steps never change again, so a client commits those labels and asks with since = stable_len.  Every
 * other position of the buffers is written as zero.  A stream without frames reports the root alone: one result of length 0.
 * Queued on `stream` behind the chunks already queued there; asynchronous (the `since` values are copied before the call returns).
 * A row that does not fit L_cap is not cut: nothing of that stream's rows is written and the next ctcd_check_status reports
 * CTCD_EINVAL (it checks the peek's status words before those of the last decode launch, which stay as they are).
 * CTCD_EINVAL: n_best < 1 or > beam, a state that is not this decoder's (device, beam), a state twice in the batch, streams with
 * different scorers.  CTCD_EUNSUPPORTED: streams behind a callback scorer (the interim result needs "<s>" / "</s>" / last-word
 * windows its cache may not hold).  The decoder and the states stay usable after every refused call. */
int ctcd_stream_peek(ctcd_decoder *dec, ctcd_stream **states, int B, int n_best, const int32_t *since_host /* [B] or NULL */,
                     int32_t *out_tokens, int32_t *out_timesteps /* DEVICE [B, n_best, L_cap] */, int L_cap,
                     float *out_scores, int32_t *out_lens /* DEVICE [B, n_best] */,
                     int32_t *n_results, int32_t *stable_lens /* DEVICE [B] */, void *stream);

/* Compaction of parked streams (extension; the reference frees a trie node as soon as no beam prefix hangs below it,
 * path_trie.cpp remove()).  A stream's node pool is append-only and sized for frames * beam + 1 nodes; the nodes a later chunk, peek
 * or stream end can reach are the ancestors of the current beam entries.  ctcd_stream_compact keeps exactly those per stream -- the
 * root, then every entry's own part of its path in beam order -- drops the rest and rewrites every stored pool index.  Nothing a
 * later call computes changes: chunks, ctcd_stream_peek and the stream-ending call give bit-identical results whether or not, how
 * often and at which chunk boundaries a stream was compacted.  live_nodes_host[b] (HOST, or NULL) receives the nodes stream b keeps
 * (1 for a stream without frames: the root; such a stream is left as it is).  Afterwards the stream's pool count is bounded by
 * live + (frames fed since) * beam (ctcd_stream_pool_nodes): the "stream too long for this beam width" refusal applies to that
 * bound, not to frames * beam.  A stream whose new need -- max(the capacity it was created with, 2 * live) nodes -- is at most a
 * quarter of its pool's capacity moves to a block of that size (ctcd_stream_bytes falls); every other stream keeps its block.
 * Queued on `stream` behind the chunks already queued there (ctcd_stream_decode calls nobody has checked yet included), and
 * synchronous: the node counts come back before the new layouts are written.  Streams behind the built-in scorer and behind a
 * callback scorer are compacted like any other (the scorer is not touched).
 * CTCD_EINVAL: a state that is not this decoder's (device) or differs from states[0] in beam or V, a state twice in the batch,
 * streams with different scorers.  CTCD_EINTERNAL: a parked state no decode wrote (that stream's block is unchanged). */
int ctcd_stream_compact(ctcd_decoder *dec, ctcd_stream **states, int B, int32_t *live_nodes_host /* [B] or NULL */, void *stream);
/* upper bound of the stream's pool count | nodes its pool holds | bytes of its HBM block (-1: st == NULL) */
long long ctcd_stream_pool_nodes(const ctcd_stream *st);
long long ctcd_stream_pool_capacity(const ctcd_stream *st);
long long ctcd_stream_bytes(const ctcd_stream *st);
/* Policy of the streaming calls on this decoder: min_nodes > 0 -- a stream whose chunk does not fit its pool and whose bound is at
 * least min_nodes is compacted first (all such streams of the call together) and grows by doubling only if the chunk still does
 * not fit; 0 (the default): it doubles, as without this call.  With the policy on, a stream's memory follows its live set. */
int ctcd_set_stream_compaction(ctcd_decoder *dec, long long min_nodes);

/* Commit of live streams' final labels (extension).  stable_len labels of every current beam entry of a stream are final
 * (ctcd_stream_peek): ctcd_stream_commit hands all of them but the last to the caller -- once -- and drops their trie nodes, the
 * committed trunk, together with the dead nodes: the node of the last committed label becomes the stream's root and the live set is
 * laid out below it as ctcd_stream_compact lays it out.  Per stream b with C_b labels committed earlier (ctcd_stream_committed) and
 * absolute stable length s_b: counts_host[b] = m_b = max(0, s_b - 1 - C_b); row b of the buffers the allocator returned holds the
 * labels and ABSOLUTE time steps at absolute depths C_b + 1 .. C_b + m_b -- row 0 of the one-shot decode of the frames fed so far at
 * those positions, past frame 65535 too -- and zeros behind them.  The allocator is called once, with (R = 1, L = the largest m_b of
 * the call; *out_L receives L), before any stream is changed; it returns two int32 buffers of B * L elements (return non-zero to
 * fail the call: nothing is committed; with L == 0 the buffers are not touched).  live_nodes_host[b] (HOST, or NULL): the nodes
 * stream b keeps.  m_b == 0 is a plain compaction of that stream; a stream without frames is left as it is.
 * From then on everything the stream reports counts from its new root: later chunks (on any kernel), ctcd_stream_compact,
 * ctcd_stream_peek (lengths, `since`, stable_lens) and the stream-ending call report the one-shot decode's rows with their first
 * C_b + m_b labels removed -- scores, result counts and row order unchanged, time steps absolute -- so committed ++ reported row is
 * the reference's row, for every row.  The library does not keep the committed labels: the caller does.  The capacity bookkeeping is
 * the compaction's (bound = live + frames since * beam, the move to a smaller block, the 2^31 bound).  A second commit with no frame
 * in between commits nothing and changes no byte.  Queued on `stream` behind the chunks already queued there, and synchronous.
 * CTCD_EINVAL as for ctcd_stream_compact.  CTCD_EUNSUPPORTED: streams with a scorer, built-in or callback (their result scores use
 * a prefix's absolute depth); no state of the call is changed.  CTCD_EINTERNAL: a parked state no decode wrote (that stream's block
 * is unchanged and nothing of it is committed). */
int ctcd_stream_commit(ctcd_decoder *dec, ctcd_stream **states, int B, ctcd_result_alloc_fn alloc, void *alloc_user,
                       int32_t *counts_host /* [B] */, int32_t *live_nodes_host /* [B] or NULL */, int *out_L /* or NULL */, void *stream);
/* labels the stream has committed so far (-1: st == NULL) */
long long ctcd_stream_committed(const ctcd_stream *st);

/* Images of live streams in host memory (extension).  ctcd_stream_save writes, per stream, one contiguous byte string that holds
 * everything the stream is: 32-bit little-endian words [16-word header: magic, format version 1, total words, beam, labels, scorer
 * kind (0 none / 1 built-in), scorer fingerprint (64 bits), frames fed (64), labels committed (64), nodes M, beam arrays A, two
 * reserved | the 12 header words of the parked state | A * beam beam-array words | M nodes of 12 bytes | M express words | M high
 * parts of the time steps]; bytes = 4 * (16 + 12 + A * beam + 5 * M) with A = 14 without a scorer and 26 with one -- a function of
 * beam, scorer kind and M alone, nothing of it depends on the block's capacity or address.  The image is canonical: saving twice
 * with no frame in between, or save -> restore -> save, gives identical bytes.
 * ctcd_stream_save HAS EXACTLY ctcd_stream_compact's EFFECT on the saved streams (an image is the layout a compaction leaves, so the
 * call compacts first; compaction changes nothing a later call computes) and changes nothing else about them: they stay live and
 * decode on.  The allocator is called once, when the sizes are known, with the size of the whole batch: image b starts at the sum
 * of the earlier images' sizes, each rounded up to a multiple of 16 bytes; bytes_out_host[b] receives image b's size.  A stream
 * without frames saves as the root alone (M = 1) and restores to a fresh stream.  Queued on `stream` behind the chunks already
 * queued there, and synchronous.
 * CTCD_EINVAL as for ctcd_stream_compact (a state twice in the batch, another decoder's state, ...), or the allocator returned NULL.
 * CTCD_EUNSUPPORTED: streams behind a callback scorer (their states index a per-process cache); nothing of them is touched.
 *
 * ctcd_stream_restore creates B new streams on `dec` from B images; stream b then behaves bit-identically to the stream image b was
 * saved from, for every later chunk (on any kernel), peek, compact, commit and stream end: committed labels, absolute frame
 * numbers, the danger flag, the speculative select's prediction and the order array travel.  `dec` may be another decoder, on
 * another device or in another process, with the same labels, beam width and blank.  scorer: NULL for images without a scorer, else
 * a built-in scorer with the image's fingerprint (a 64-bit hash of its tables and of order, char_based, space_id and dictionary size;
 * alpha / beta are not part of it).  Every image is validated on the host before anything is allocated or uploaded (magic, version,
 * size, beam / labels / scorer against the call, every index a kernel follows, and the node layout against the image's own depth
 * and LCP arrays): the call is all or nothing -- if one image is refused (CTCD_EINVAL; ctcd_last_error names the item and the
 * check) no stream is created and nothing stays allocated.  The restored stream's capacity is max(frames_hint frames (0: 1024),
 * 2 * M nodes), its bound M + frames since * beam: as after a compaction.  Synchronous. */
typedef void *(*ctcd_bytes_alloc_fn)(void *user, unsigned long long bytes);
int ctcd_stream_save(ctcd_decoder *dec, ctcd_stream **states, int B, ctcd_bytes_alloc_fn alloc, void *alloc_user,
                     unsigned long long *bytes_out_host /* [B] */, void *stream);
int ctcd_stream_restore(ctcd_decoder *dec, ctcd_scorer *scorer /* or NULL */, const void *const *blobs /* [B] HOST */,
                        const unsigned long long *bytes /* [B] */, int B, int frames_hint, ctcd_stream **out_states /* [B] */, void *stream);
/* What an image says about itself; needs no device (a router can look at an image without a GPU).  CTCD_EINVAL: not an image
 * (NULL, too short, wrong magic / version, or a size that is not the one its own beam / scorer kind / node count give). */
typedef struct ctcd_snapshot_info_t {
  int32_t version, beam, labels, scorer_kind, nodes, reserved;
  long long frames, committed;
  unsigned long long fingerprint, bytes;
} ctcd_snapshot_info_t;
int ctcd_snapshot_info(const void *blob, unsigned long long bytes, ctcd_snapshot_info_t *info);
/* the fingerprint images saved behind this scorer carry (0: NULL or a callback scorer) */
unsigned long long ctcd_scorer_fingerprint(const ctcd_scorer *scorer);

/* Host check of the per-item status words written by the last ctcd_beam_decode (synchronises the device). */
int ctcd_check_status(ctcd_decoder *dec, int B);
/* ... without blocking: enqueues the copy of the B status words (0 = ok) into `host_status` (page-locked memory) on
 * `stream` -- the launch stream, before anything else is enqueued there; the caller synchronises on its own event.  For
 * pipelined callers that queue the next batch before looking at this one. */
int ctcd_fetch_status_async(ctcd_decoder *dec, int B, int32_t *host_status, void *stream);

/* Vocabulary prune bookkeeping of the last ctcd_beam_decode (0 for the no-prune configurations).  A frame in which equal
 * values sit at the cutoff_top_n boundary or among the kept ones is ordered by whatever std::sort does with the whole
 * row (decoder_utils.cpp:19-20), and a cumulative sum next to cutoff_prob depends on the reference's sequential chain of
 * binary64 log / exp (decoder_utils.cpp:25-32): those frames are "flagged" by the fast prune pass and settled by a second
 * device kernel that replays libstdc++'s std::sort and walks the chain with bit-exact restatements of glibc's log / exp
 * (exact_math_f64.h).  Nothing reaches the host toolchain since round 4: ctcd_last_prune_host_rows is always 0.
 * ctcd_last_prune_flagged_rows waits for the call's stream (the count arrives behind the kernels). */
long long ctcd_last_prune_flagged_rows(ctcd_decoder *dec);
long long ctcd_last_prune_host_rows(ctcd_decoder *dec);

/* HIP-event timing of the decode kernel alone (events recorded on the launch stream). */
int ctcd_set_timing(ctcd_decoder *dec, int on);
int ctcd_last_kernel_ms(ctcd_decoder *dec, float *ms);
int ctcd_last_prune_ms(ctcd_decoder *dec, float *ms); /* the vocabulary-prune kernel of the same call (pruned configurations) */
int ctcd_last_resolve_ms(ctcd_decoder *dec, float *ms); /* ... and what follows it up to the decode kernel: the flagged frames' replay */

/* Test hook: device expf/logf/log_sum_exp (exact_math.h; modes 0..2) and binary64 log / exp / log_sum_exp<double>
 * (exact_math_f64.h; modes 3: log(p), 4: log(p + FLT_MIN), 5: exp(x) over float bit patterns, 6: pairs) vs the host C library. */
int ctcd_debug_math_check(ctcd_decoder *dec, int mode, uint32_t lo, uint32_t hi, uint32_t stride, const float *xs,
                          const float *ys, long long n_pairs, long long *checked, long long *mismatches);

/* Test/tuning hook: instrumented build of the kernel; out = int64 [B][16] per-phase timer ticks. */
int ctcd_debug_set_profile(ctcd_decoder *dec, int on);
int ctcd_debug_get_profile(ctcd_decoder *dec, long long *out, int B);
/* Test hook: 1 (default) = beams <= 128 over <= 32 labels run the kernel variant with a compile-time workspace layout,
 * 0 = always the run-time layout (identical results). */
int ctcd_debug_set_fixed_layout(ctcd_decoder *dec, int on);
/* Test hook: 1 (default) = the std::sort replay of flagged prune frames works in LDS when the row fits, 0 = always in
 * global memory, the path of rows beyond ~11 000 labels (identical results). */
int ctcd_debug_set_prune_resolve(ctcd_decoder *dec, int on);
/* Test hook for log_input == 2: 1 (default) = rows of more than 256 labels (a multiple of four) are normalised by a workgroup
 * each, and in front of a vocabulary prune not at all -- one kernel reads the logits and emits the kept candidates' normalised
 * values; 0 = always the one-wave log_softmax pass followed by the separate prune (identical results). */
int ctcd_debug_set_fused_logits(ctcd_decoder *dec, int on);
/* Test hook: the workgroup form of the vocabulary-prune pass (rows of 257 .. 10 240 labels, a multiple of four, cutoff_top_n <= 64) keeps
 * the row in registers between its two looks at it (1, default) or reads it twice (0: the form of rounds 2-5).  Identical results. */
int ctcd_debug_set_prune_registers(ctcd_decoder *dec, int on);
/* Test hook: the vocabulary-prune pass's output of the last call (get_pruned_log_probs, decoder_utils.cpp:10-45, per frame), copied
 * to HOST memory: cnt[rows], labels / values [rows][stride], stride = min(cutoff_top_n, V); entries at or beyond a frame's count
 * are unspecified.  Waits for the launch stream. */
int ctcd_debug_prune_rows(ctcd_decoder *dec, long long rows, int stride, int32_t *cnt, int32_t *labels, float *values);
/* Tuning aid (instrumented build): per-wave shader-clock stamps at every workgroup barrier of batch item 0 during frames
 * [frame0, frame0 + nframes).  out == NULL arms the following decodes; out != NULL (int64 [16][ctcd_debug_timeline_cap()])
 * fetches the stamps, arrival and departure alternating, in program order (tools/barrier_timeline.py). */
int ctcd_debug_timeline_cap(void);
int ctcd_debug_timeline(ctcd_decoder *dec, int frame0, int nframes, long long *out);
/* Debug aid (instrumented build): beam of batch item 0 after every frame, int32 [T][1 + 4*beam] = n, then
 * (node, depth, lcp, score bits) per entry.  Call with on=1 before a decode, then with out != NULL to fetch. */
int ctcd_debug_beam_dump(ctcd_decoder *dec, int on, int *out, int T, int beam);

/* Test hook for the host-tensor entry points (ctcd_beam_decode_to_host / _host / _lm_host): input_streaming = 0 / 1 turns
 * the streamed input off / on (-1: leave; on by default: the kernel is launched before its rows have crossed PCIe and
 * waits for them frame block by frame block; 2: on, but the "frames arrived" counter is never advanced -- the kernel must
 * give up after about a second and the call repeat itself the plain way); mirror_cap_labels >= 0 shrinks the page-locked mirror a finished utterance
 * copies its compact results into (utterances beyond it are fetched from the device buffer afterwards; -1: default size,
 * -2: leave). */
int ctcd_debug_set_host_path(ctcd_decoder *dec, int input_streaming, long long mirror_cap_labels);

/* Half-precision input.  After ctcd_set_input_dtype(dec, CTCD_DTYPE_F16 or CTCD_DTYPE_BF16) every entry point of `dec` that
 * takes `probs` / `logits` reads them as [B, T, V] IEEE binary16 / bfloat16 elements (device memory; the pointer keeps its
 * `const float *` spelling), until the dtype is set again.  Widening to float32 is exact: the results are those of the same
 * call on the float32 copy, bit for bit, without that copy -- the pre-passes (vocabulary prune, log_softmax, prob -> log) read
 * the half rows themselves; where a decode kernel reads the caller's rows (no pruning, or the LM tier) one widening pass
 * writes float32 rows into the decoder's workspace.  Host-memory input stays float32: ctcd_beam_decode_to_host with
 * probs_on_device == 0 (and so the *_host entry points) returns CTCD_EUNSUPPORTED while a half dtype is set.
 * ctcd_log_softmax's output stays float32, and with a half dtype `out` must not overlap `logits` (CTCD_EINVAL: in-place is float32
 * only).  The dtype is state of `dec`, like ctcd_set_threads: threads that share a decoder and pass different dtypes must not let
 * a set-and-call pair of one overlap a call of the other (a half buffer read as float32 is read twice its size).
 * ctcd_last_input_dtype: the dtype the last call of `dec` read its rows as. */
#define CTCD_DTYPE_F32 0
#define CTCD_DTYPE_F16 1
#define CTCD_DTYPE_BF16 2
int ctcd_set_input_dtype(ctcd_decoder *dec, int dtype);
int ctcd_last_input_dtype(ctcd_decoder *dec);

/* Launch order.  A launch lasts as long as its slowest workgroup, and once a batch outnumbers the workgroups the device holds at
 * once (256 CUs; 512 with two per CU) the rest start as slots free up: a long utterance that starts late runs on alone.
 * CTCD_ORDER_LENGTH makes the workgroups take their utterances longest first: a small pass on the call's stream sorts the
 * clamped seq_lens (descending, ties in batch order; NULL seq_lens: every length is T) without a copy to the host, and each
 * workgroup, as it starts, draws a ticket and decodes the utterance of that rank.  Results stay where they are and are
 * bit-identical to batch order; with ctcd_set_timing the kernel time includes the sort (14 us at B = 1024, 0.15 ms at 16384; above
 * 16384 items a ranking pass whose cost grows with B^2: 0.5 ms at 20000, about 50 ms at 200 000).  CTCD_ORDER_BATCH (default): workgroup i
 * decodes utterance i.  The mode is state of `dec` and applies to every one-shot entry point (ctcd_beam_decode, _host, _to_host,
 * _compact, _lm, _lm_host); with a callback scorer also to its resumed launches, ordered by the frames each utterance has left.
 * Streaming calls (ctcd_stream_*) keep batch order, and so do the wide-beam run-time layouts (ctcd_debug_last_layout 4-6).
 * Anything but the two modes, or a NULL decoder: CTCD_EINVAL.
 * ctcd_debug_last_launch_order (tests): copies the permutation of the last one-shot call -- with a callback scorer, of its first
 * launch -- into out[B] (B must be that call's batch size) and returns 1, or returns 0 if that call ran in batch order. */
#define CTCD_ORDER_BATCH 0
#define CTCD_ORDER_LENGTH 1
int ctcd_set_launch_order(ctcd_decoder *dec, int mode);
int ctcd_debug_last_launch_order(ctcd_decoder *dec, int32_t *out, int B);

/* ---- Blank-frame filter (no reference counterpart): drop the frames whose blank posterior exceeds a threshold BEFORE the beam
 * search, on the device, and map the reported time steps back afterwards.  A launch lasts as long as its slowest utterance
 * walks its frames; CTC posteriors put almost all mass on blank in most frames.  Three calls a C user composes around any
 * one-shot decode (INTEGRATION.md has the recipe); no existing entry point knows about them.
 *
 * ctcd_blank_skip: for utterance b with n = seq_lens[b] clamped to [0, T] (seq_lens NULL: T), frame t < n is SKIPPED iff v > cmp,
 * v = the float32 value of x[b][t][blank_id] (the element type follows ctcd_set_input_dtype; a half element is widened exactly).
 * The compare is ordered and strict: NaN is kept, a value equal to cmp is kept; frames at or beyond n are never read.  The caller
 * chooses cmp for its rows: the threshold itself for probabilities, its logarithm for log-probabilities (raw logits: run
 * ctcd_log_softmax first and filter its float32 output).  Writes
 *   out_kept int32 [B][T]   out_kept[b][i] = original index of the i-th kept frame, in order; 0 from out_lens[b] on
 *   out_lens int32 [B]      the number of kept frames
 *   out_rows [B][T][V]      of x's element type: rows [b][0 .. out_lens[b]) = the kept rows in order, the rest unspecified;
 *                           must not be x (an in-place filter is not offered)
 * A decode of out_rows with seq_lens = out_lens is the decode of the kept frames.
 * ctcd_remap_timesteps: out_timesteps[b][p][i] = kept[b][out_timesteps[b][p][i]] for i < out_lens[b][p] (read on the device), in
 * place on the padded [B, K, T] tensor; a word that is no index below kept_lens[b] is left as it is.
 * ctcd_remap_compact: the same on compact results -- the frame half (upper 16 bits) of every label record the entries of c_ent
 * own, inside each item's range of c_hdr; T <= 65536 as for compact delivery.  Expanding the remapped records gives the remapped
 * padded tensors.
 * ctcd_remap_timesteps_host: ctcd_remap_timesteps on HOST tensors (all four pointers host memory), valid prefixes only, items
 * spread over num_threads threads; synchronous; needs no decoder.  `kept` is a map ctcd_blank_skip wrote (strictly increasing per
 * utterance): an utterance none of whose frames was skipped is recognised by its last entry and its rows are not touched.
 * The device calls are asynchronous on `stream`.  Every call refuses a NULL pointer (seq_lens excepted) and B, T, V or K <= 0 with
 * CTCD_EINVAL before it touches the device. */
int ctcd_blank_skip(ctcd_decoder *dec, const void *x, const int32_t *seq_lens, int B, int T, int V, int blank_id, float cmp,
                    void *out_rows, int32_t *out_lens, int32_t *out_kept, void *stream);
int ctcd_remap_timesteps(ctcd_decoder *dec, int32_t *out_timesteps, const int32_t *out_lens, const int32_t *kept,
                         const int32_t *kept_lens, int B, int K, int T, void *stream);
int ctcd_remap_compact(ctcd_decoder *dec, const int32_t *c_hdr, const int32_t *c_ent, uint32_t *c_labels, const int32_t *kept,
                       const int32_t *kept_lens, int B, int K, int T, void *stream);
int ctcd_remap_timesteps_host(int32_t *out_timesteps, const int32_t *out_lens, const int32_t *kept, const int32_t *kept_lens, int B,
                              int K, int T, int num_threads);

/* ---- Blank-frame filter of live streams (no reference counterpart): the same filter in front of every chunk of the streams of a
 * decoder.  ctcd_set_stream_blank_skip(dec, on, cmp_prob, cmp_log) is state of `dec` (off by default; off leaves every streaming
 * call exactly as it is): cmp_prob is the float32 bound for log_input == 0, cmp_log the one for log_input == 1 and 2 (the threshold
 * and its logarithm, rounded to float32 by the caller; NaN is CTCD_EINVAL).
 *
 * Definition.  A stream's SEEN frames are the valid frames of all chunks fed so far, probs[b, :clamp(seq_lens_host[b], 0, T)] of each
 * call in order.  Seen frame s is skipped iff its blank value v > cmp (ctcd_blank_skip's compare: ordered, strict, NaN kept, equality
 * kept, a half element widened exactly; log_input == 2: v is the blank entry of ctcd_log_softmax of the row).  The stream decodes the
 * kept frames alone, and every time step it reports is the kept frame's index among the seen frames: the stream-ending call, and
 * ctcd_stream_peek (results, `since`, stable_lens count labels as ever) and ctcd_stream_commit (the returned labels' time steps, and
 * everything reported afterwards).  So, however the frames were cut into chunks, a stream returns what the one-shot decode of the
 * concatenation behind ctcd_blank_skip returns -- tokens, scores, lengths, result counts and time steps, bit for bit.  A chunk whose
 * frames are all skipped feeds nothing (also when it ends the stream); a stream whose frames were all skipped ends with the root alone.
 *
 * With the filter on, ctcd_stream_decode, ctcd_stream_decode_to_host, ctcd_stream_peek and ctcd_stream_commit do all of it inside the
 * one call, on the caller's stream: log-softmax first for raw logits (float32; the rows are then filtered and decoded as
 * log-probabilities), scan and gather into decoder-owned scratch, the decode of the kept rows with the kept counts as chunk lengths,
 * the remap of whatever the call reports.  seq_lens_host is a host array and the node pools are sized from it on the host: A FILTERED
 * CHUNK CALL WAITS FOR `stream` until the B kept counts have arrived, before it launches its decode -- one small read per call, which
 * costs a stream synchronisation (ctcd_stream_decode is no longer asynchronous up to that point; what it queues behind is).
 * Each stream owns a frame map in device memory, int32, 4 bytes per kept frame (map[i] = seen-index of the i-th kept frame): an
 * allocation of its own beside the stream's block, made with the stream (room for the frames its pool starts with), grown by doubling
 * on the stream the chunks are queued on, freed with the stream,
 * never shrunk (ctcd_stream_compact and ctcd_stream_commit leave it alone); ctcd_stream_map_bytes reports it.
 * ctcd_stream_frames keeps its meaning -- the frames the stream has DECODED, the kept ones: pool bounds, the 2^31 refusal, out_T
 * (>= the kept frames of an ending stream) and ctcd_set_stream_compaction count those -- and ctcd_stream_frames_seen reports the seen
 * frames (for a stream that never met the filter: the same number).  frames, frames seen and the map's used length advance together,
 * and only when the decode launch was accepted: a refused call leaves the stream as it was (map entries written beyond `frames` are
 * overwritten by the next call).  ctcd_last_stream_blank_skip: frames considered and kept by the last filtered chunk call.
 * Compact delivery holds 16-bit frame numbers: with the filter on ctcd_stream_decode_to_host serves a call only while
 * frames seen + T <= 65536 for every stream of it (the records are remapped on the device and fetched from there; no page-locked
 * mirror); beyond that it returns CTCD_EUNSUPPORTED and the streams end through ctcd_stream_decode, whose padded tensors are remapped
 * on the device.
 * Restrictions.  A stream adopts the filter at its first chunk: a stream that has frames under the other setting is CTCD_EINVAL on
 * ctcd_stream_decode / _to_host / _peek / _commit, and nothing changes.  ctcd_stream_save of a filtered stream and
 * ctcd_stream_restore on a decoder with the filter on are CTCD_EUNSUPPORTED (the image format has no place for the map); the
 * refused streams stay live and decode on.  Streams with the built-in scorer and behind a callback scorer take the filter like any
 * other (ctcd_stream_peek behind a callback scorer stays refused).
 * ctcd_last_stream_blank_skip_ms (with ctcd_set_timing): HIP-event time of the last filtered chunk call's filter (log-softmax, scan,
 * gather), host time of its wait for the kept counts, HIP-event time of the remap behind it (0 where none ran). */
int ctcd_set_stream_blank_skip(ctcd_decoder *dec, int on, float cmp_prob, float cmp_log);
long long ctcd_stream_frames_seen(const ctcd_stream *st); /* -1: st == NULL */
long long ctcd_stream_map_bytes(const ctcd_stream *st);   /* -1: st == NULL */
int ctcd_last_stream_blank_skip(ctcd_decoder *dec, long long *considered, long long *kept);
int ctcd_last_stream_blank_skip_ms(ctcd_decoder *dec, float *filter_ms, float *wait_ms, float *remap_ms);

/* ---- n-best results (no reference counterpart): rows 0 .. n-1 of every item alone.  The one-shot entry points above return all
 * `beam` rows -- two padded [B, beam, T] tensors -- and almost every caller reads row 0 or a handful.  With 1 <= n_best <= beam:
 *   out_tokens, out_timesteps int32 [B][n_best][T]     out_scores float [B][n_best]     out_lens int32 [B][n_best]
 * equal to rows [:, :n_best] of the full call's tensors, bit for bit, and defined everywhere: label positions at or beyond a
 * row's length are 0; a row at or beyond the item's result count has length 0, score 0 and zero labels.  n_results (optional)
 * receives every item's FULL result count.  n_best outside [1, beam] is CTCD_EINVAL; nothing is launched.
 *
 * ctcd_expand_compact_nbest: compact records (c_hdr / c_ent of stride `beam` / c_labels, n_labels = the words c_labels holds) ->
 * the [B, n_best, T] pair.  All device memory, asynchronous on `stream`; beam <= 4096 as for ctcd_expand_compact, T <= 65536.
 * Every record index is checked before it is followed -- the item's range of c_hdr against n_labels, an entry's labels against the
 * item's range, its row against beam, its lengths against T and its trie predecessor.  A malformed record zeroes the rows that
 * would have drawn labels from it and RAISES the item's word of `status` (B device words the caller has zeroed, or NULL) to
 * CTCD_NBEST_BAD_RECORD; words of well-formed items are not written.
 * ctcd_beam_decode_nbest: ctcd_beam_decode / ctcd_beam_decode_lm (scorer may be NULL) with the four [B, n_best, ...] DEVICE tensors
 * out; asynchronous on `stream`, nothing is read back in between.  The decode writes compact records into decoder-owned scratch
 * and the n-best expansion follows on the same stream; a malformed record raises the item's decode status word
 * (ctcd_check_status).  The scratch belongs to the decoder's next call: queue that call on the same stream, or wait.
 * ctcd_beam_decode_to_host_nbest: ctcd_beam_decode_to_host with [B, n_best, ...] HOST tensors: the records cross PCIe compact and
 * are mirrored as there, the host threads expand the rows below n_best alone, and their number follows B x n_best x T.
 * Where the compact form is not to be had -- T > 65536, T == 0, a callback scorer -- the call decodes in full on the device and
 * delivers rows [:, :n_best] (on the host route only those cross PCIe): whatever the full call decodes, the n-best call decodes. */
#define CTCD_NBEST_BAD_RECORD 7
int ctcd_expand_compact_nbest(ctcd_decoder *dec, const int32_t *c_hdr, const int32_t *c_ent, const uint32_t *c_labels, long long n_labels,
                              int B, int beam, int T, int n_best, int32_t *out_tokens, int32_t *out_timesteps, int32_t *status, void *stream);
int ctcd_beam_decode_nbest(ctcd_decoder *dec, const float *probs, const int32_t *seq_lens, int B, int T, int V, int beam, int num_processes,
                           double cutoff_prob, int cutoff_top_n, int blank_id, int log_input, ctcd_scorer *scorer, int n_best,
                           int32_t *out_tokens, int32_t *out_timesteps, float *out_scores, int32_t *out_lens, int32_t *n_results, void *stream);
int ctcd_beam_decode_to_host_nbest(ctcd_decoder *dec, const float *probs, const int32_t *seq_lens, int probs_on_device, int B, int T, int V,
                                   int beam, int num_processes, double cutoff_prob, int cutoff_top_n, int blank_id, int log_input,
                                   ctcd_scorer *scorer, int n_best, int32_t *out_tokens, int32_t *out_timesteps, float *out_scores,
                                   int32_t *out_lens, int32_t *n_results, void *stream);

/* ---- Forced alignment (no reference counterpart): for the rows a caller keeps, the frames each label occupies on the best CTC path
 * of the row through the item's acoustic rows, and that path's score -- a Viterbi score that does not depend on what the beam search
 * pruned.  (out_timesteps of a decode is something else: the frame at which the search first appended the label.)
 *
 * Definition.  For item b: n = clamp(seq_lens[b], 0, T) (T when seq_lens is NULL).  lp(t, c) is the float32 log-probability of
 * label c at frame t, as the decoder's input mode defines it:
 *   log_input == 1: the input value, a half value widened exactly.
 *   log_input == 0: float(log(double(p) + FLT_MIN)), the value prob_to_log_kernel computes.
 *   log_input == 2: the value ctcd_log_softmax writes.
 * A hypothesis y[0..L) has the extended sequence z of S = 2L + 1 states: z[2i] = blank_id, z[2i+1] = y[i].  The recurrence:
 *   d[0][0] = lp(0, blank).   d[0][1] = lp(0, y[0]) (if L >= 1).   d[0][s] = -inf otherwise.
 *   d[t][s] = lp(t, z[s]) + max(d[t-1][s], d[t-1][s-1], d[t-1][s-2]).
 *     The third predecessor is allowed only for odd s >= 3 with z[s] != z[s-2].  A predecessor index below 0 does not exist.
 *   The addition is one float32 addition; the maximum is exact.
 *   Back-pointer: the allowed predecessor with the greatest value; among equals the one with the largest state index (stay, before
 *   s-1, before s-2).
 *   End state: the greater of d[n-1][S-1] and d[n-1][S-2] (S-2 only if L >= 1).  On equality the end state is S-1.
 * The result: `score` is that end value.  The path is traced back from there.  start[i] and end[i] are the first and last frame,
 * inclusive, that the path spends in state 2i+1.
 * The special cases:
 *   A hypothesis with score == -inf or n == 0 with L > 0 is NOT ALIGNED.  This covers L > n, repeats that do not fit, and rows of
 *   -inf.  Its score is -inf and its spans are 0.
 *   L == 0 and n >= 1: the score is the sum of the blank's lp over the n frames in frame order, and there are no spans.
 *   L == 0 and n == 0: score 0.
 *   NaN inputs are undefined, as for the beam search.
 * Every position of the outputs at or beyond a row's length is written as 0.
 * The validity rules: a label outside [0, V), a label equal to blank_id, or a length outside [0, L_stride] makes the row INVALID.  An
 * invalid row's outputs are zeroed and its score is 0.  The item's word of `status` is raised to CTCD_ALIGN_BAD_ROW.  Nothing is
 * ever read through an unchecked index.
 *
 * ctcd_ctc_align: everything is device memory and asynchronous on `stream`.  probs [B][T][V] has the dtype ctcd_set_input_dtype set
 * (f32 / f16 / bf16, widened exactly as everywhere else).  tokens int32 [B][R][L_stride], lens int32 [B][R]: with L_stride = T the
 * call takes a device decode's out_tokens and out_lens as they are, R = beam or n_best.  out_start, out_end int32 [B][R][L_stride],
 * out_scores float [B][R].  status: B device words the caller has zeroed, or NULL; words of items without an invalid row are not
 * written.  log_input == 2 runs the log-softmax pass into decoder-owned float32 scratch first; log_input == 0 converts the values it
 * gathers with the device's restated binary64 log and makes no converted copy of the input.  The back-pointers (2 bits per frame and
 * state) live in decoder-owned scratch cut into slots of the worst-case size for (T, min(L_stride, T)); min(B x R, budget / slot
 * bytes) persistent workgroups -- at least one -- take the rows in turn, so nothing of `lens` is read on the host and no
 * allocation grows with B x R.  The scratch belongs to the decoder's next alignment: queue that call on the same stream, or wait.
 * CTCD_EINVAL for bad shapes (negative sizes, V < 1, blank_id outside [0, V), log_input outside 0 .. 2, a NULL tensor), and nothing is
 * launched.  CTCD_EUNSUPPORTED: min(L_stride, T) > 2047 (an extended sequence beyond the 4096 states one workgroup holds).
 * ctcd_set_align_scratch: the budget of the back-pointer scratch in bytes; 0 = the default (256 MiB).
 * ctcd_last_align_grid: the workgroups the last ctcd_ctc_align launched (0: none yet; -1: dec == NULL). */
#define CTCD_ALIGN_BAD_ROW 8
int ctcd_ctc_align(ctcd_decoder *dec, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input,
                   const int32_t *tokens /* [B][R][L_stride] */, const int32_t *lens /* [B][R] */, int R, int L_stride,
                   int32_t *out_start, int32_t *out_end /* [B][R][L_stride] */, float *out_scores /* [B][R] */,
                   int32_t *status /* [B] zeroed by the caller, or NULL */, void *stream);
int ctcd_set_align_scratch(ctcd_decoder *dec, long long bytes);   /* budget of the back-pointer scratch; 0 = the default */
long long ctcd_last_align_grid(const ctcd_decoder *dec);

/* ---- CTC log-likelihood (no reference counterpart): for the rows a caller keeps, log P(y | x) -- the sum over ALL alignments of
 * the row through the item's acoustic rows, by the forward algorithm.  It is the quantity CTC defines: it does not depend on what
 * the beam search pruned (as the decode's scores do) and is not the single best alignment's share (as ctcd_ctc_align's score is),
 * so it is what n-best rescoring, confidence estimates and comparisons between decoders are built on.  exp of it is the model's
 * posterior of the transcript; log-likelihood - alignment score >= 0 is how much of that mass lies outside the best alignment.
 *
 * Definition.  n, lp(t, c) for the three log_input modes, the extended sequence z and S = 2L + 1 are exactly those of "Forced
 * alignment"; so is the third predecessor: allowed only for odd s >= 3 with z[s] != z[s-2].
 * lse3(v0, v1, v2), the three-way float32 log-sum-exp; an absent argument counts as -inf:
 *   m = max(v0, v1, v2), exact.  If m == -inf the result is -inf.
 *   Otherwise the result is logf((expf(v0 - m) + expf(v1 - m)) + expf(v2 - m)) + m.
 *     Every operation is one float32 operation, and the sum is taken in that order.
 *     expf and logf are glibc's (2.35, the FMA variants; csrc/exact_math.h expf_nonpos / logf_normal restate them on the domains
 *     that occur: <= 0 for the exponential, [1, 3] for the logarithm).  expf(0) = 1 exactly and expf(-inf) = 0.
 *     logf(..) + m is always evaluated: a cell with one finite predecessor m yields +0 + m, which for m = -0.0 is +0.0.
 *     An implementation may replace the maximum's own term by 1.0f and skip -inf terms (bit-identical); it may not reorder the sum
 *     or skip the logf.
 * The recurrence:
 *   a[0][0] = lp(0, blank).   a[0][1] = lp(0, y[0]) (if L >= 1).   a[0][s] = -inf otherwise.
 *   a[t][s] = lp(t, z[s]) + lse3(a[t-1][s], a[t-1][s-1], a[t-1][s-2]), one float32 addition.  Predecessors that do not exist or
 *   are not allowed count as -inf.
 * The result: ll = lse3(a[n-1][S-1], a[n-1][S-2] (if L >= 1), -inf).
 * The special cases:
 *   n == 0: ll = 0 for L == 0, -inf otherwise.
 *   L > n: -inf, and no recurrence runs.
 *   NaN and +inf inputs are undefined.  -inf inputs and sums that overflow to -inf follow from the rules above.
 * The validity rules are those of "Forced alignment": a label outside [0, V), a label equal to blank_id, or a length outside
 * [0, L_stride] makes the row INVALID.  An invalid row's output is 0, and the item's word of `status` is raised to
 * CTCD_ALIGN_BAD_ROW (the same value, the same meaning).  Nothing is ever read through an unchecked index.
 *
 * ctcd_ctc_loglik: everything is device memory and asynchronous on `stream`; nothing of `lens` is read on the host.  probs, tokens,
 * lens and status are as for ctcd_ctc_align -- with L_stride = T the call takes a device decode's out_tokens and out_lens as they
 * are -- and out_loglik is float [B][R].  log_input == 2 runs the log-softmax pass into the decoder-owned float32 rows that
 * ctcd_ctc_align uses too: they belong to the decoder's next alignment or log-likelihood, so queue that call on the same stream, or
 * wait.  log_input == 0 converts the values it gathers and makes no converted copy of the input.  There is no other scratch: a
 * row's states live in registers.  Rows are classed as the alignment's (groups of four one-wave rows side by side; any other row on
 * a workgroup with 1, 4 or 16 states per lane), one launch per class the shape allows; each takes min(units, cap) persistent
 * workgroups, the cap being by default the workgroups the device holds at once (compute units x the occupancy the class's registers
 * allow).  The error codes are ctcd_ctc_align's: CTCD_EINVAL for bad shapes (negative sizes, V < 1, blank_id outside [0, V),
 * log_input outside 0 .. 2, a NULL tensor), and nothing is launched; CTCD_EUNSUPPORTED for min(L_stride, T) > 2047, V > 2^28 or more
 * than 2^31 - 1 rows.  B x R == 0 is CTCD_OK and launches nothing.  Streams are out of scope: score the concatenated rows one-shot.
 * ctcd_set_loglik_grid: the cap of every launch's grid; 0 = the default.  The results do not depend on it.
 * ctcd_last_loglik_grid: the widest grid the last ctcd_ctc_loglik launched (0: none yet; -1: dec == NULL). */
int ctcd_ctc_loglik(ctcd_decoder *dec, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input,
                    const int32_t *tokens /* [B][R][L_stride] */, const int32_t *lens /* [B][R] */, int R, int L_stride,
                    float *out_loglik /* [B][R] */, int32_t *status /* [B] zeroed by the caller, or NULL */, void *stream);
int ctcd_set_loglik_grid(ctcd_decoder *dec, long long max_workgroups);   /* 0 = the default */
long long ctcd_last_loglik_grid(const ctcd_decoder *dec);

/* ---- Label posteriors (no reference counterpart): CTC forward-backward for the rows a caller keeps, reduced to three numbers per
 * label -- where the label's posterior peaks, how many frames it is expected to occupy, and how much the frames that carry it vote
 * for it -- next to the row's log-likelihood.  One number per row cannot say which label of a transcript is shaky; these can.
 *
 * Definition.  n, lp(t, c), the extended sequence z, S = 2L + 1, the allowed skip, lse3 and a[t][s] are exactly those of "CTC
 * log-likelihood".  Every operation below is one float32 operation, in the order written; all arithmetic is IEEE float32 with
 * subnormals, and the division is correctly rounded.
 *   ll: the result of "CTC log-likelihood".
 *   beta:
 *     b[n-1][S-1] = lp(n-1, blank).   b[n-1][S-2] = lp(n-1, y[L-1]) (if L >= 1).   b[n-1][s] = -inf otherwise.
 *     b[t][s] = lp(t, z[s]) + lse3(b[t+1][s], b[t+1][s+1], b[t+1][s+2]).
 *       The third argument is present only for odd s with s + 2 <= S - 1 and z[s+2] != z[s]; an index beyond S - 1 does not exist.
 *     This is a of the reversed labels over the frames n-1 .. 0.
 *   e80(x): if x > 0, x is taken as 0.  If x < -80 the value is 0.0f.  Otherwise the value is glibc's expf(x) (csrc/exact_math.h
 *     expf_nonpos).  The cut at -80 keeps e80 itself out of the subnormal range; the clamp at 0 takes in the last-place excess that
 *     rounding gives a + b - lp - ll.
 *   g[t], for label i with s = 2i + 1:
 *     g[t] = 0 if a[t][s] or b[t][s] is -inf, or their float sum is.
 *     Otherwise g[t] = e80(((a[t][s] + b[t][s]) - lp(t, z[s])) - ll).
 *   occupancy[i]: the float32 sum of g[t] taken in the order t = n-1, n-2, .., 0, starting from +0.0.
 *   num[i]: the same sum of g[t] * e80(lp(t, z[s])); the product is one float32 multiplication and may be subnormal.
 *   confidence[i] = num[i] / occupancy[i], one IEEE-rounded division; 0 if occupancy[i] == 0.  It lies in [0, 1].
 *   peaks[i]: the smallest t whose g[t] equals the greatest.
 * The special cases:
 *   A row with ll == -inf, L > n or n == 0 has all per-label outputs 0; its loglik is as "CTC log-likelihood" defines it.
 *   Every position of the per-label outputs at or beyond a row's length is written as 0.
 *   NaN and +inf inputs are undefined.
 * The validity rules are those of "Forced alignment": an INVALID row has all outputs 0, and the item's word of `status` is raised to
 * CTCD_ALIGN_BAD_ROW.  Nothing is ever read through an unchecked index.
 *
 * ctcd_ctc_posteriors: everything is device memory and asynchronous on `stream`; nothing of `lens` is read on the host.  probs,
 * tokens, lens and status are as for ctcd_ctc_align.  out_peaks int32, out_occupancy and out_confidence float, each
 * [B][R][L_stride]; out_loglik float [B][R], bit for bit what ctcd_ctc_loglik writes.  log_input == 2 runs the log-softmax pass into
 * the decoder-owned float32 rows the alignment uses too.  A row is walked twice, forward and backward; between the walks a lives in
 * decoder-owned scratch cut into slots of max(T x (2 min(L_stride, T) + 1), T x 256) floats, rounded up to 256 bytes; min(B x R,
 * budget / slot bytes) persistent workgroups -- at least one -- take the rows in turn, and only grid x slot bytes are allocated.
 * The scratch belongs to the decoder's next call of this function: queue it on the same stream, or wait.  The error codes are
 * ctcd_ctc_align's: CTCD_EINVAL for bad shapes, and nothing is launched; CTCD_EUNSUPPORTED for min(L_stride, T) > 2047, V > 2^28 or
 * more than 2^31 - 1 rows.  B x R == 0 is CTCD_OK and launches nothing.  Streams are out of scope.
 * ctcd_set_posterior_scratch: the budget of that scratch in bytes; 0 = the default (2 GiB: one workgroup per compute unit at
 * T = L_stride = 1000).  The results do not depend on it.
 * ctcd_last_posterior_grid: the workgroups the last ctcd_ctc_posteriors launched (0: none yet; -1: dec == NULL). */
int ctcd_ctc_posteriors(ctcd_decoder *dec, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input,
                        const int32_t *tokens /* [B][R][L_stride] */, const int32_t *lens /* [B][R] */, int R, int L_stride,
                        int32_t *out_peaks, float *out_occupancy, float *out_confidence /* [B][R][L_stride] */,
                        float *out_loglik /* [B][R] */, int32_t *status /* [B] zeroed by the caller, or NULL */, void *stream);
int ctcd_set_posterior_scratch(ctcd_decoder *dec, long long bytes);   /* budget of the scratch; 0 = the default */
long long ctcd_last_posterior_grid(const ctcd_decoder *dec);

/* ---- Greedy decode (no reference counterpart; the reference's test file defines a greedy_result it never uses): the best-path
 * decode -- every frame's most probable label, repeats collapsed, blanks dropped -- in one read of the input.  No beam, no language
 * model, no vocabulary prune and no blank-frame filter take part.
 *
 * Definition.  For item b: n = clamp(seq_lens[b], 0, T) (T when seq_lens is NULL).  x(t, c) is the input value of label c at frame
 * t, a half value widened exactly.  lp(t, c) is exactly the lp of "Forced alignment" for log_input 0, 1 and 2.
 * The frame label:
 *   c*(t) is the index of the greatest x(t, .).  The compare is an ordered, strict `>` walked from c = 0: among equal values the
 *   smallest index wins, -0.0 and +0.0 are equal, and a frame of all -inf gives 0.
 *   This holds in all three input modes: the winner is chosen on the input values, not on lp.
 *   NaN inputs are undefined, as elsewhere.  Nothing is read or written out of bounds because of one.
 * The emission:
 *   Frame t < n emits label c*(t) iff c*(t) != blank_id and (t == 0 or c*(t) != c*(t-1)).
 *   The emitted labels in frame order are tokens[0..L).  starts[i] is the emitting frame.  ends[i] is the last frame of that run of
 *   equal c*.
 *   label_scores[i] is the greatest lp(t, c*(t)) over starts[i] .. ends[i].  The maximum is exact and involves no arithmetic; where
 *   -0.0 and +0.0 are both the greatest, it is the one of the earlier frame.
 * The score:
 *   n == 0: score 0 and L = 0.
 *   Otherwise score = lp(0, c*(0)), then score = score + lp(t, c*(t)) for t = 1 .. n-1 in that order.  Each step is one float32
 *   addition.  The sign is that of ctcd_ctc_align's score (a log-probability), not the sign convention of a decode's out_scores.
 * lp(t, c*(t)) by mode:
 *   log_input == 1: x(t, c*(t)).
 *   log_input == 0: float(log(double(p) + FLT_MIN)) of the winner only.
 *   log_input == 2: the value ctcd_log_softmax would write there.  With the frame's NaN-skipping maximum m (a zero maximum taken as
 *   +0) that is (x - m) - logf(s), the sum s taken in the order that function's definition fixes: 64 chains j mod 64 in increasing j,
 *   then the butterfly.  For m = -inf it is -inf.  No [B][T][V] copy of the input is written.
 * Every output position at or beyond L is written as 0.
 * What follows: float32 addition is monotone in both arguments and c*(t) carries the greatest lp of its frame, so no path sums to
 * more than the greedy one -- ctcd_ctc_align of the greedy row returns a score with equal bits (log_input 1 and 2; log_input 0 as far
 * as the restated binary64 log is monotone).
 *
 * ctcd_greedy_decode: everything is device memory and asynchronous on `stream`; nothing is read on the host.  probs [B][T][V] has the
 * dtype ctcd_set_input_dtype set.  out_tokens, out_starts int32 [B][T]; out_ends int32 [B][T] and out_label_scores float [B][T], or
 * NULL each; out_scores float [B], out_lens int32 [B].  out_tokens / out_lens are rows ctcd_ctc_align, ctcd_ctc_loglik and
 * ctcd_ctc_posteriors take with R = 1, L_stride = T.  Two kernels run behind each other: an argmax pass that leaves c*(t) and
 * lp(t, c*(t)) of every frame below n in decoder-owned scratch (8 bytes per frame), and a collapse pass, one workgroup per item.  The
 * scratch belongs to the decoder's next greedy decode: queue that call on the same stream, or wait.  A decoder built with a scorer
 * ignores it.  CTCD_EINVAL for bad shapes (negative sizes, V < 1, blank_id outside [0, V), log_input outside 0 .. 2, a NULL tensor),
 * and nothing is launched.  CTCD_EUNSUPPORTED for V > 2^28.  B == 0 is CTCD_OK and launches nothing; T == 0 with B > 0 writes
 * out_lens and out_scores as zeros.  More than one row per item and host pointers are out of scope; streams: the next section. */
int ctcd_greedy_decode(ctcd_decoder *dec, const void *probs, const int32_t *seq_lens, int B, int T, int V, int blank_id, int log_input,
                       int32_t *out_tokens, int32_t *out_starts /* [B][T] */, int32_t *out_ends, float *out_label_scores /* [B][T] or NULL */,
                       float *out_scores, int32_t *out_lens /* [B] */, void *stream);

/* ---- Greedy decode of live streams: "Greedy decode" of a stream whose frames arrive chunk by chunk.  Under best-path decoding a
 * label is final the moment its frame has been seen, so a call returns final labels, nothing is revised, and what a stream keeps
 * between calls is a record of 32 bytes.
 *
 * Definition.  A greedy stream is created with a first frame number F0 >= 0.  A call feeds stream b the chunk probs[b, :n_b],
 * n_b = clamp(seq_lens[b], 0, Tc) (Tc when seq_lens is NULL), and carries a host flag is_eos[b].
 * The concatenation:
 *   X is all frames fed to the stream so far, this chunk included; N is their count before this call.
 *   tokens, starts, ends, label_scores, score, L are what "Greedy decode" defines for X (one item, n = its frame count).
 *   Every frame number is reported shifted by F0.
 * What a call returns for stream b:
 *   out_tokens[b][0..E) and out_starts[b][0..E) are the labels of X whose emitting frame lies in this chunk, in order;
 *   E = out_lens[b] <= n_b.
 *   out_scores[b] is the score of X.  A stream that has never had a frame has score 0.0f.  The first frame ever seen sets the
 *   score to its lp (a first lp of -0.0 stays -0.0); every later frame is one float32 addition, across calls as within them.
 *   out_ends[b][0..C) and out_label_scores[b][0..C), C = out_closed_lens[b], are the ends / label_scores of the runs of X whose last
 *   frame became known in this call, in order: the run with last frame e (unshifted) is reported by the first call for which
 *   N + n_b > e + 1, or is_eos[b] and N + n_b == e + 1.  A run that reaches the chunk's last frame of a stream that goes on stays
 *   open: its maximum so far travels in the record and a later call closes it -- a call with n_b == 0 and is_eos too.  Over a
 *   stream's life the i-th closed run belongs to the i-th emitted label.  Up to n_b + 1 runs close in one call (the carried one and
 *   n_b new ones): these two outputs have Tc + 1 columns.
 *   The tie rule of the run maximum holds across calls: among equal values (-0.0, +0.0) the earlier frame's wins, also when that
 *   frame was in an earlier call.
 *   Every output position at or beyond its count is written as 0.
 * What follows: however a row is cut into chunks, the calls' outputs concatenated are the row's ctcd_greedy_decode outputs, and the
 * last call's score is its score, with equal bits.
 *
 * ctcd_greedy_stream_create / _destroy: a stream and its record on the decoder's device.  ctcd_greedy_stream_reset: a fresh stream
 * with a first frame number again, the record written by a kernel queued on `stream`.  first_frame outside [0, 2^31 - 1] is
 * CTCD_EINVAL.
 * ctcd_greedy_stream_decode: states and is_eos are host arrays [B]; everything else is device memory and asynchronous on `stream`;
 * nothing is read on the host.  probs [B][Tc][V] has the dtype ctcd_set_input_dtype set; the three input modes are those of
 * ctcd_greedy_decode, whose argmax pass runs on the chunk as it stands, with the same decoder-owned frame records (they, and the
 * staged per-stream arguments, belong to the decoder's next greedy call: queue it on the same stream, or wait).  out_tokens,
 * out_starts int32 [B][Tc]; out_ends int32 [B][Tc + 1], out_label_scores float [B][Tc + 1] and out_closed_lens int32 [B], or NULL
 * each; out_scores float [B], out_lens int32 [B].  Tc == 0 is legal: it writes the counts and the running score, and closes the open
 * run of a stream whose is_eos is set.  No scorer, prune or blank filter takes part.
 * CTCD_EINVAL, and nothing is launched: bad shapes, blank_id, log_input and NULL tensors as for ctcd_greedy_decode; a stream that has
 * ended (is_eos in an earlier call) and was not reset; the same stream twice in one call; a stream of another device.
 * CTCD_EUNSUPPORTED, and nothing is launched: the host keeps an upper bound of a stream's frame numbers, F0 + the Tc of every call,
 * and a call that would take it beyond 2^31 - 1 is refused; the stream is intact.  V > 2^28.  B == 0 is CTCD_OK and launches nothing.
 * ctcd_greedy_stream_info: waits for the device, then out = {frames fed (exact, unshifted), labels emitted, runs closed, 1 if a run
 * is open else 0}.
 * More than one row per item, host-pointer entry points and save / restore of a greedy stream are out of scope. */
typedef struct ctcd_greedy_stream ctcd_greedy_stream;
int ctcd_greedy_stream_create(ctcd_decoder *dec, ctcd_greedy_stream **out, long long first_frame);
void ctcd_greedy_stream_destroy(ctcd_decoder *dec, ctcd_greedy_stream *st);
int ctcd_greedy_stream_reset(ctcd_decoder *dec, ctcd_greedy_stream *st, long long first_frame, void *stream);
int ctcd_greedy_stream_decode(ctcd_decoder *dec, ctcd_greedy_stream **states, const unsigned char *is_eos /* HOST [B] */,
                              const void *probs, const int32_t *seq_lens, int B, int Tc, int V, int blank_id, int log_input,
                              int32_t *out_tokens, int32_t *out_starts /* [B][Tc] */, int32_t *out_ends,
                              float *out_label_scores /* [B][Tc + 1] or NULL */, int32_t *out_closed_lens /* [B] or NULL */,
                              float *out_scores, int32_t *out_lens /* [B] */, void *stream);
int ctcd_greedy_stream_info(ctcd_decoder *dec, const ctcd_greedy_stream *st, long long out[4]); /* waits */

/* ---- Edit distance (no reference counterpart): how far apart two label rows are -- the Levenshtein distance between the rows a
 * caller keeps and reference rows, or between all rows of an item.  It is what an error rate, the oracle row of an n-best list and
 * minimum-Bayes-risk selection are built on.  The arithmetic is integer: the definition is exact and equality is equality.
 *
 * Definition.  lev(a, b) is the unit-cost Levenshtein distance between two int32 sequences: the least number of insertions, deletions
 * and substitutions, each of cost 1, that turn a into b; a match costs 0.  lev(a, []) = len(a).
 *   Elements are compared as int32 values and nothing else: every int32 is a token, negative values and blank_id among them.  No
 *   vocabulary takes part, so word ids give word-level distances.
 * The inputs: x int32 [B][R][L] with x_lens [B][R]; y int32 [B][Q][Lq] with y_lens [B][Q].
 * The output: out int32 [B][R][Q], out[b][i][j] = lev(x[b][i][:x_lens[b][i]], y[b][j][:y_lens[b][j]]).
 * Pairwise mode is selected by y == NULL: y is x and Q = R (the Q, Lq and y_lens passed are ignored).
 *   The diagonal is written as 0.  Only the pairs i < j are computed; each result is written to both [i][j] and [j][i].
 * Positions of a row at or beyond its length are never read.
 * The validity rule: a length outside [0, L] (y: outside [0, Lq]) raises the item's word of `status` to CTCD_ALIGN_BAD_ROW (the same
 * value, the same meaning), and ALL outputs of that item are 0.  Nothing is ever read through an unchecked length.
 *
 * ctcd_edit_distance: everything is device memory and asynchronous on `stream`; nothing is read on the host.  status: B device words
 * the caller has zeroed, or NULL; words of valid items are not written.  One wave takes one pair: of the pair's two rows the shorter
 * is held in the wave's registers, up to 32 columns per lane, and the longer is streamed past it -- lev is symmetric, so the choice
 * is made per pair on the device, and the limit is one of tensor dimensions alone.
 * CTCD_EINVAL, and nothing is launched: negative sizes, or a NULL tensor that is needed (x_lens, out; x when L > 0; y_lens when y is
 * given).  B == 0, R == 0 or Q == 0 is CTCD_OK and launches nothing.  L == 0 or Lq == 0 is legal: the distances are the other side's
 * lengths (in the general mode y must still be a non-NULL pointer; it is not read).
 * CTCD_EUNSUPPORTED: min(L, Lq) > 2048 (pairwise mode: L > 2048); the longer side is bounded only by 2^30 positions per row, and B x R
 * and B x Q by 2^31 - 1.
 * ctcd_last_edit_pairs: the distances the last ctcd_edit_distance computed -- B x R x Q in the general mode, B x R x (R - 1) / 2 in
 * pairwise mode (0: none yet, or an empty call; -1: dec == NULL).
 * ctcd_set_edit_grid: the most workgroups (of four waves, a pair each) the launch uses; 0 = the default, two per compute unit.  The
 * results do not depend on it; with a grid of one, four waves take all pairs in turn.  ctcd_last_edit_grid: the workgroups the last
 * ctcd_edit_distance launched (0: none yet, or an empty call; -1: dec == NULL).
 * Not provided: sharing the common prefix of a beam's rows.  (The counts of the edits and the alignment: the next section.) */
int ctcd_edit_distance(ctcd_decoder *dec, const int32_t *x /* [B][R][L] */, const int32_t *x_lens /* [B][R] */, int B, int R, int L,
                       const int32_t *y /* [B][Q][Lq], or NULL: pairwise */, const int32_t *y_lens /* [B][Q] */, int Q, int Lq,
                       int32_t *out /* [B][R][Q] */, int32_t *status /* [B] zeroed by the caller, or NULL */, void *stream);
long long ctcd_last_edit_pairs(const ctcd_decoder *dec);
int ctcd_set_edit_grid(ctcd_decoder *dec, long long max_workgroups);   /* 0 = the default */
long long ctcd_last_edit_grid(const ctcd_decoder *dec);

/* ---- Edit operations (no reference counterpart): how an edit distance splits into substitutions, deletions and insertions -- the
 * breakdown of an error-rate report -- and which token of a hypothesis stands against which token of a reference.  Integer
 * arithmetic throughout, exact like "Edit distance", whose comparison of tokens (int32 values, nothing else), inputs, modes, validity
 * rule and status word are used here unchanged.
 *
 * Definition.  x is the hypothesis row, of lx tokens; y is the reference row, of ly tokens.  An alignment is a monotone path from
 * (0, 0) to (lx, ly) made of three kinds of step:
 *   a pair (i, j) -> (i+1, j+1): a HIT if x[i] == y[j], a SUBSTITUTION otherwise;
 *   an x-only step (i, j) -> (i+1, j): x[i] has no partner, an INSERTION;
 *   a y-only step (i, j) -> (i, j+1): y[j] has no partner, a DELETION.
 * Its key is the tuple (D, S): D the number of substitutions, insertions and deletions, S the number of substitutions.
 * The optimal key is the lexicographically least one: the least distance, and among the alignments of that distance the fewest
 *   substitutions.  Since H = (lx + ly - D - S) / 2, that is the most hits.  D is lev(x, y) of "Edit distance".
 *   The order is translation-invariant and both components add up along a path, so the cell recurrence
 *   K[i][j] = min(K[i-1][j-1] + (x[i-1] != y[j-1] ? (1,1) : (0,0)), K[i-1][j] + (1,0), K[i][j-1] + (1,0)),
 *   K[0][j] = (j, 0), K[i][0] = (i, 0), is exact.
 * The counts (H, S, Del, I) of an optimal alignment follow from K[lx][ly] = (D, S) and the lengths alone:
 *   I = (D - S + lx - ly) / 2, Del = (D - S - lx + ly) / 2, H = lx - S - I.
 *   They do not depend on which optimal path is taken.  Exchanging x and y exchanges I and Del and leaves H and S as they are.
 *   H + S + I == lx, H + S + Del == ly, S + Del + I == lev(x, y).
 * The canonical alignment is found by walking back from (lx, ly).  At (i, j):
 *   1. if i > 0 and j > 0 and K[i-1][j-1] + the pair's cost == K[i][j], take the pair;
 *   2. otherwise, if i > 0 and K[i-1][j] + (1,0) == K[i][j], take the insertion (x-only);
 *   3. otherwise take the deletion.
 *   The preference is one of x and y: which of the two rows the device keeps in registers does not enter.
 *   x = [a, b], y = [b, a]: D = 2, S = 0, x_to_y = [1, -1], y_to_x = [-1, 0].
 * The packed form the device computes with is K = D * 4096 + S in one 32-bit word: S <= min(lx, ly) <= 2048 < 4096, and the key and
 *   every candidate stay below 2^31 while max(L, Lq) <= 262144.
 *
 * ctcd_edit_counts: the arguments, modes, validity rule, status word and error codes of ctcd_edit_distance; out int32 [B][R][Q][4] =
 * (H, S, Del, I).  Pairwise mode (y == NULL): [i][j] takes row i as x; [j][i] is the same with Del and I exchanged; the diagonal is
 * (len, 0, 0, 0).  An invalid item: all words 0.  One more limit: max(L, Lq) > 262144 is CTCD_EUNSUPPORTED.  ctcd_set_edit_grid,
 * ctcd_last_edit_pairs and ctcd_last_edit_grid apply to it (and to ctcd_edit_align) as to ctcd_edit_distance.
 *
 * ctcd_edit_align: the general mode only; y == NULL is CTCD_EINVAL.  x_to_y int32 [B][R][Q][L]: x_to_y[..][p] is the index of x[p]'s
 * partner in y on the canonical alignment, or -1 if x[p] is an insertion, and -1 for p >= lx.  y_to_x int32 [B][R][Q][Lq] is the same
 * from the other side (-1: a deletion, or beyond ly).  counts [B][R][Q][4] as above, or NULL.  Every word of all three is written; an
 * invalid item has all maps -1 and all counts 0.  Everything is device memory and asynchronous on `stream`; nothing is read on the
 * host.  The limits are those of ctcd_edit_counts.
 * The directions of the walk, two bits per cell, live in decoder-owned scratch: one slot per wave in flight, of max(L, Lq) rows of 64
 * words -- 4 bytes each while min(L, Lq) <= 1024, 8 bytes beyond -- sized from the tensor dimensions alone.  The launch has as many
 * waves as the usual grid, as the call has pairs, or as the budget has slots for, whichever is least; only that many slots are
 * allocated, when first needed.  If one slot does not fit the budget the call returns CTCD_EUNSUPPORTED, the sizes in
 * ctcd_last_error, and the decoder stays usable.  The scratch belongs to the decoder's next ctcd_edit_align: queue it on the same
 * stream, or wait.
 * ctcd_set_edit_scratch: that budget in bytes; 0 = the default, 1 GiB.  The results do not depend on it.
 * ctcd_last_edit_slots: the slots (waves with a pair to work on) of the last ctcd_edit_align (0: none yet, or an empty call; -1:
 * dec == NULL).
 * Not provided: alignments in pairwise mode, weighted costs, and sharing the common prefix of a beam's rows. */
int ctcd_edit_counts(ctcd_decoder *dec, const int32_t *x /* [B][R][L] */, const int32_t *x_lens /* [B][R] */, int B, int R, int L,
                     const int32_t *y /* [B][Q][Lq], or NULL: pairwise */, const int32_t *y_lens /* [B][Q] */, int Q, int Lq,
                     int32_t *out /* [B][R][Q][4] = H, S, Del, I */, int32_t *status /* [B] zeroed by the caller, or NULL */, void *stream);
int ctcd_edit_align(ctcd_decoder *dec, const int32_t *x /* [B][R][L] */, const int32_t *x_lens /* [B][R] */, int B, int R, int L,
                    const int32_t *y /* [B][Q][Lq] */, const int32_t *y_lens /* [B][Q] */, int Q, int Lq,
                    int32_t *x_to_y /* [B][R][Q][L] */, int32_t *y_to_x /* [B][R][Q][Lq] */, int32_t *counts /* [B][R][Q][4], or NULL */,
                    int32_t *status /* [B] zeroed by the caller, or NULL */, void *stream);
int ctcd_set_edit_scratch(ctcd_decoder *dec, long long bytes);   /* budget of the back-pointer scratch; 0 = the default */
long long ctcd_last_edit_slots(const ctcd_decoder *dec);

/* Tuning / introspection. */
int ctcd_set_threads(ctcd_decoder *dec, int threads_per_workgroup); /* 0 = automatic (default); else a power of two in [64, 1024] */
/* Two workgroups per CU.  The fixed-layout class (beam <= 128, <= 32 labels) has a second build of its kernel that fits
 * two utterances on a compute unit (<= 64 VGPRs; the exact replay's scratch in HBM: 67 KB of LDS instead of 132 KB): a lone
 * workgroup runs ~7 % slower in it, two on a CU together 1.4-1.5x faster.  mode = -1 (default): used when a batch has
 * more utterances than the device has CUs; 1: always (a serving loop that keeps several launches in flight); 0: never. */
int ctcd_set_cu_sharing(ctcd_decoder *dec, int mode);
/* Exact-shape kernels.  The plain north-star build (beam <= 128, <= 32 labels, no pruning, no scorer, 1024 threads, one workgroup per
 * CU, rows resident on the device) has twins cut for ONE shape each, in which beam width, label count and blank index are constants
 * of the frame loop: today beam 100 over 29 labels with the blank at index 0 -- the reference's default beam_width over the English
 * grapheme set.  Results are bit-identical.  mode = -1 (default): a twin runs wherever a whole-utterance call has exactly its shape
 * (not streams, not resumed launches, not rows streamed from the host, not when another build of the class is planned); 0: never;
 * 1: required -- a call that does not qualify returns CTCD_EUNSUPPORTED and launches nothing.  ctcd_last_exact_shape: whether the
 * last launch ran a twin (0 / 1; -1: dec == NULL).  ctcd_debug_last_kernel / _layout keep reporting the planned kernel. */
int ctcd_set_exact_shape(ctcd_decoder *dec, int mode);
int ctcd_last_exact_shape(const ctcd_decoder *dec);
/* The north-star class of shapes (beam <= 128, <= 32 labels, no scorer) has a second build of its kernel whose phase A1 settles
 * four subtrees per wavefront at once: beams shaped like chains -- what blank-dominated rows, i.e. real acoustic posteriors,
 * produce: some twenty entries with descendants in the beam per frame -- decode 7 % faster with it, bushy beams (random rows:
 * one or two) 3 % slower.  mode -1 (default): chosen per launch from the shape statistic of the last launch whose status was
 * checked (ctcd_check_status; the *_host / to_host entries check); 0 / 1: never / always.  Results are identical in both
 * builds (mode 1 in a library built without the subtree build: CTCD_EUNSUPPORTED).  ctcd_last_subtree_search: which build the
 * last launch used (0 / 1). */
int ctcd_set_subtree_search(ctcd_decoder *dec, int mode);
int ctcd_last_subtree_search(const ctcd_decoder *dec);
/* The workspace layout of the kernel the last decode launch used (tests prove with it which kernel ran): 0 = the run-time layout;
 * 1 = the fixed layout (beam <= 128, <= 32 labels); 2 = the pruned default's compile-time layout (beam <= 112, <= 40 candidates of
 * <= 10240 labels, 1024 threads, no scorer: its rank table is tagged with the frame mod 1024); 3 = the first wide-beam layout at its
 * compile-time size (beam <= 500, <= 29 labels, no pruning); 4 / 5 / 6 = the run-time layout with HBM scratch at level 1 / 2 / 3
 * (wide beams; level 3: more than 65535 candidate slots).  -1: no launch yet. */
int ctcd_debug_last_layout(const ctcd_decoder *dec);
/* The kernel instantiation the last decode launch used (tests prove with it that every instantiation is reached): writes its
 * template arguments {PROF, BIG, LAYOUT, PRUNED, NT, LM, OCC2} (decode_kernel.h CTC_KERNEL_LIST; LM as 0 / 1 / 2 / 3, the others
 * as 0 / 1 or their value) to params[7] and returns CTCD_OK.  A launch that failed is not recorded (nor by ctcd_debug_last_layout
 * and ctcd_last_subtree_search).  -1 (CTCD_EINVAL): no launch yet, or a NULL argument (that case alone sets ctcd_last_error). */
int ctcd_debug_last_kernel(const ctcd_decoder *dec, int32_t params[7]);
/* The pre-pass kernels the last call of `dec` launched (tests prove with it that every pre-pass instantiation is reached): four stages
 * -- elementwise (prob -> log / half rows widened), log_softmax, vocabulary prune, prune_resolve_kernel -- of four words each, {kernel,
 * a, b, dtype}: kernel one of CTCD_PP_* (CTCD_PP_NONE: the stage launched nothing, and the other three words are 0); a = F4 of the
 * workgroup kernels, R of prune_rows_kernel, else 0; b = REG of prune_rows_wg_kernel, for prune_resolve_kernel its route (0: arrays in
 * LDS, 1: in global memory, ctcd_debug_set_prune_resolve), else 0; dtype = the CTCD_DTYPE_* the kernel reads.  A stage is recorded once
 * its launch is queued; every decode call (and ctcd_log_softmax) that reaches its pre-passes starts with four empty stages.
 * ctcd_debug_prepass_table: every pre-pass instantiation of the build, five words each {kernel, a, b, dtype, largest V the dispatch sends
 * to it or 0: no bound}, up to `cap` of them written to `out`; returns their number. */
#define CTCD_PP_NONE 0
#define CTCD_PP_PROB_TO_LOG 1   /* prob_to_log_kernel<DT> */
#define CTCD_PP_WIDEN 2         /* widen_rows_kernel<DT> */
#define CTCD_PP_LSM_WAVE 3      /* log_softmax_rows_kernel<DT> (one wave per row) */
#define CTCD_PP_LSM_WG 4        /* log_softmax_rows_wg_kernel<F4, DT> */
#define CTCD_PP_PRUNE_ROWS 5    /* prune_rows_kernel<R, DT> */
#define CTCD_PP_PRUNE_WG 6      /* prune_rows_wg_kernel<F4, REG, DT> */
#define CTCD_PP_PRUNE_LOGITS 7  /* prune_logits_wg_kernel<F4, DT> (raw logits -> candidates) */
#define CTCD_PP_RESOLVE 8       /* prune_resolve_kernel<DT> */
#define CTCD_PREPASS_FIELDS 16
int ctcd_debug_last_prepass(const ctcd_decoder *dec, int32_t out[CTCD_PREPASS_FIELDS]);
int ctcd_debug_prepass_table(int32_t *out, int cap);
int ctcd_workgroup_lds_bytes(int beam, int V, int cutoff_top_n, double cutoff_prob); /* LDS one utterance needs (default build) */
const char *ctcd_last_error(void);
const char *ctcd_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CTCDECODE_AMD_H_ */
