"""ctypes binding of the C ABI in include/ctcdecode_amd.h (the only way the Python layer reaches the decoder).

There is NO CPU fallback: if the HIP library is missing or does not load, importing this module raises.
"""
import ctypes
import os

from . import _build

_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)

# ctcd_cond_log10_fn (include/ctcdecode_amd.h): int fn(void *user, const char *const *words, int n, float *log10_prob)
COND_LOG10_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, _f32p)
# ctcd_cond_log10_batch_fn: int fn(void *user, const char *const *words, int n_windows, int order, float *log10_probs, int32_t *status)
COND_LOG10_BATCH_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int, _f32p,
                                       ctypes.POINTER(ctypes.c_int32))

# ctcd_result_alloc_fn: int fn(void *user, int R, int L, int32_t **tokens, int32_t **timesteps)
RESULT_ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p))
# ctcd_bytes_alloc_fn: void *fn(void *user, unsigned long long bytes)
BYTES_ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong)


class SnapshotInfo(ctypes.Structure):  # ctcd_snapshot_info_t
    _fields_ = [("version", ctypes.c_int32), ("beam", ctypes.c_int32), ("labels", ctypes.c_int32), ("scorer_kind", ctypes.c_int32),
                ("nodes", ctypes.c_int32), ("reserved", ctypes.c_int32), ("frames", ctypes.c_longlong), ("committed", ctypes.c_longlong),
                ("fingerprint", ctypes.c_ulonglong), ("bytes", ctypes.c_ulonglong)]

SYMBOLS = ["ctcd_log_softmax", "ctcd_compact_label_capacity", "ctcd_beam_decode_compact", "ctcd_expand_compact", "ctcd_beam_decode_to_host", "ctcd_scorer_create", "ctcd_scorer_destroy", "ctcd_scorer_is_character_based", "ctcd_scorer_max_order", "ctcd_scorer_dict_size",
           "ctcd_scorer_reset_params", "ctcd_scorer_cond_log_prob", "ctcd_scorer_create_callback", "ctcd_scorer_cond_log10", "ctcd_scorer_callback_calls", "ctcd_scorer_callback_seconds", "ctcd_scorer_set_callback_threads", "ctcd_scorer_create_callback_batch", "ctcd_scorer_cond_log10_batch", "ctcd_scorer_callback_batches", "ctcd_beam_decode_lm", "ctcd_beam_decode_lm_host", "ctcd_stream_create_lm",
           "ctcd_create", "ctcd_destroy", "ctcd_beam_decode", "ctcd_beam_decode_host", "ctcd_check_status", "ctcd_fetch_status_async", "ctcd_stream_create", "ctcd_stream_destroy", "ctcd_stream_frames", "ctcd_stream_decode", "ctcd_stream_decode_to_host", "ctcd_stream_peek", "ctcd_stream_compact", "ctcd_stream_commit", "ctcd_stream_committed", "ctcd_stream_save", "ctcd_stream_restore", "ctcd_snapshot_info", "ctcd_scorer_fingerprint", "ctcd_stream_pool_nodes", "ctcd_stream_pool_capacity", "ctcd_stream_bytes", "ctcd_set_stream_compaction", "ctcd_last_prune_host_rows", "ctcd_last_prune_flagged_rows", "ctcd_last_scorer_rounds", "ctcd_last_scorer_waits", "ctcd_set_scorer_wait", "ctcd_set_scorer_filter", "ctcd_last_scorer_pairs",
           "ctcd_set_threads", "ctcd_set_cu_sharing", "ctcd_set_exact_shape", "ctcd_last_exact_shape", "ctcd_set_input_dtype", "ctcd_last_input_dtype", "ctcd_set_launch_order", "ctcd_debug_last_launch_order", "ctcd_set_subtree_search", "ctcd_last_subtree_search", "ctcd_debug_last_layout", "ctcd_debug_last_kernel", "ctcd_debug_last_prepass", "ctcd_debug_prepass_table", "ctcd_debug_set_host_path", "ctcd_set_timing", "ctcd_last_kernel_ms", "ctcd_last_prune_ms", "ctcd_last_resolve_ms", "ctcd_debug_math_check", "ctcd_debug_set_profile", "ctcd_debug_set_fixed_layout", "ctcd_debug_set_prune_resolve", "ctcd_debug_set_fused_logits", "ctcd_debug_set_prune_registers", "ctcd_debug_prune_rows", "ctcd_debug_timeline", "ctcd_debug_timeline_cap", "ctcd_debug_get_profile", "ctcd_debug_beam_dump", "ctcd_workgroup_lds_bytes", "ctcd_last_error", "ctcd_version",
           "ctcd_blank_skip", "ctcd_remap_timesteps", "ctcd_remap_compact", "ctcd_remap_timesteps_host",
           "ctcd_set_stream_blank_skip", "ctcd_stream_frames_seen", "ctcd_stream_map_bytes", "ctcd_last_stream_blank_skip", "ctcd_last_stream_blank_skip_ms",
           "ctcd_expand_compact_nbest", "ctcd_beam_decode_nbest", "ctcd_beam_decode_to_host_nbest",
           "ctcd_ctc_align", "ctcd_set_align_scratch", "ctcd_last_align_grid",
           "ctcd_ctc_loglik", "ctcd_set_loglik_grid", "ctcd_last_loglik_grid",
           "ctcd_ctc_posteriors", "ctcd_set_posterior_scratch", "ctcd_last_posterior_grid",
           "ctcd_greedy_decode",
           "ctcd_greedy_stream_create", "ctcd_greedy_stream_destroy", "ctcd_greedy_stream_reset", "ctcd_greedy_stream_decode", "ctcd_greedy_stream_info",
           "ctcd_edit_distance", "ctcd_last_edit_pairs", "ctcd_set_edit_grid", "ctcd_last_edit_grid",
           "ctcd_edit_counts", "ctcd_edit_align", "ctcd_set_edit_scratch", "ctcd_last_edit_slots"]


def _load():
    path = _build.LIB_PATH
    if not os.path.exists(path):
        raise ImportError("ctcdecode_amd: HIP library %s is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or `python ctcdecode_amd/_build.py`). There is no CPU fallback." % path)
    import torch  # noqa: F401  (loads the HIP runtime the library must share with PyTorch-ROCm)

    lib = ctypes.CDLL(path)
    lib.ctcd_last_error.restype = ctypes.c_char_p
    lib.ctcd_version.restype = ctypes.c_char_p
    lib.ctcd_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    lib.ctcd_destroy.argtypes = [ctypes.c_void_p]
    lib.ctcd_destroy.restype = None
    lib.ctcd_set_threads.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_set_cu_sharing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_set_exact_shape.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_last_exact_shape.argtypes = [ctypes.c_void_p]
    lib.ctcd_set_input_dtype.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_last_input_dtype.argtypes = [ctypes.c_void_p]
    lib.ctcd_set_launch_order.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_debug_last_launch_order.argtypes = [ctypes.c_void_p, _i32p, ctypes.c_int]
    lib.ctcd_set_subtree_search.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_last_subtree_search.argtypes = [ctypes.c_void_p]
    lib.ctcd_debug_last_layout.argtypes = [ctypes.c_void_p]
    lib.ctcd_debug_last_kernel.argtypes = [ctypes.c_void_p, _i32p]
    lib.ctcd_debug_last_prepass.argtypes = [ctypes.c_void_p, _i32p]
    lib.ctcd_debug_prepass_table.argtypes = [_i32p, ctypes.c_int]
    lib.ctcd_debug_set_host_path.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong]
    lib.ctcd_log_softmax.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.ctcd_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.ctcd_last_prune_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.ctcd_last_resolve_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.ctcd_debug_math_check.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    lib.ctcd_debug_set_profile.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_debug_set_fixed_layout.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_debug_set_prune_resolve.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_debug_set_fused_logits.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_debug_set_prune_registers.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_debug_prune_rows.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.ctcd_debug_timeline.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.ctcd_debug_beam_dump.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.ctcd_debug_get_profile.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_last_scorer_rounds.argtypes = [ctypes.c_void_p]
    lib.ctcd_last_scorer_waits.argtypes = [ctypes.c_void_p]
    lib.ctcd_set_scorer_wait.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_last_scorer_rounds.restype = ctypes.c_int
    lib.ctcd_last_prune_host_rows.argtypes = [ctypes.c_void_p]
    lib.ctcd_last_prune_host_rows.restype = ctypes.c_longlong
    lib.ctcd_last_prune_flagged_rows.argtypes = [ctypes.c_void_p]
    lib.ctcd_last_prune_flagged_rows.restype = ctypes.c_longlong
    lib.ctcd_stream_create.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.ctcd_stream_destroy.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.ctcd_stream_destroy.restype = None
    lib.ctcd_stream_frames.argtypes = [ctypes.c_void_p]
    lib.ctcd_stream_frames.restype = ctypes.c_longlong
    lib.ctcd_stream_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.ctcd_stream_decode_to_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               RESULT_ALLOC_FN, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
    lib.ctcd_stream_peek.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.ctcd_stream_compact.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.ctcd_stream_commit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, RESULT_ALLOC_FN, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]
    lib.ctcd_stream_save.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, BYTES_ALLOC_FN, ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong),
                                     ctypes.c_void_p]
    lib.ctcd_stream_restore.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int,
                                        ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]
    lib.ctcd_snapshot_info.argtypes = [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.POINTER(SnapshotInfo)]
    lib.ctcd_scorer_fingerprint.argtypes = [ctypes.c_void_p]
    lib.ctcd_scorer_fingerprint.restype = ctypes.c_ulonglong
    for name in ("ctcd_stream_pool_nodes", "ctcd_stream_pool_capacity", "ctcd_stream_bytes", "ctcd_stream_committed"):
        getattr(lib, name).argtypes = [ctypes.c_void_p]
        getattr(lib, name).restype = ctypes.c_longlong
    lib.ctcd_set_stream_compaction.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.ctcd_check_status.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_fetch_status_async.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.ctcd_workgroup_lds_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]
    common = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
              ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
              ctypes.c_void_p, ctypes.c_void_p]
    lib.ctcd_beam_decode.argtypes = common + [ctypes.c_void_p]
    lib.ctcd_beam_decode_host.argtypes = common
    lm_common = common[:12] + [ctypes.c_void_p] + common[12:]  # `scorer` sits before the outputs (binding.cpp:122-140)
    lib.ctcd_beam_decode_lm.argtypes = lm_common + [ctypes.c_void_p]
    lib.ctcd_beam_decode_lm_host.argtypes = lm_common
    lib.ctcd_compact_label_capacity.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.ctcd_compact_label_capacity.restype = ctypes.c_longlong
    lib.ctcd_beam_decode_compact.argtypes = common[:12] + [ctypes.c_void_p] * 5 + [ctypes.c_longlong] + [ctypes.c_void_p] * 4
    lib.ctcd_expand_compact.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3
    lib.ctcd_beam_decode_to_host.argtypes = common[:3] + [ctypes.c_int] + common[3:12] + [ctypes.c_void_p] + common[12:] + [ctypes.c_void_p]
    lib.ctcd_scorer_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_double, ctypes.c_double, ctypes.c_char_p,
                                       ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int]
    lib.ctcd_scorer_destroy.argtypes = [ctypes.c_void_p]
    lib.ctcd_scorer_destroy.restype = None
    for name in ("ctcd_scorer_is_character_based", "ctcd_scorer_max_order", "ctcd_scorer_dict_size"):
        getattr(lib, name).argtypes = [ctypes.c_void_p]
    lib.ctcd_scorer_reset_params.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double]
    lib.ctcd_scorer_cond_log_prob.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int]
    lib.ctcd_scorer_cond_log_prob.restype = ctypes.c_double
    lib.ctcd_scorer_create_callback.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                                ctypes.c_int, COND_LOG10_FN, ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int]
    lib.ctcd_scorer_cond_log10.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, _f32p]
    lib.ctcd_scorer_callback_calls.argtypes = [ctypes.c_void_p]
    lib.ctcd_scorer_callback_calls.restype = ctypes.c_longlong
    lib.ctcd_scorer_callback_seconds.argtypes = [ctypes.c_void_p]
    lib.ctcd_scorer_callback_seconds.restype = ctypes.c_double
    lib.ctcd_scorer_set_callback_threads.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_scorer_set_callback_threads.restype = ctypes.c_int
    lib.ctcd_scorer_create_callback_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                                      ctypes.c_int, COND_LOG10_BATCH_FN, ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int]
    lib.ctcd_scorer_cond_log10_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_int, _f32p, ctypes.POINTER(ctypes.c_int32)]
    lib.ctcd_scorer_callback_batches.argtypes = [ctypes.c_void_p]
    lib.ctcd_scorer_callback_batches.restype = ctypes.c_longlong
    lib.ctcd_set_scorer_filter.argtypes = [ctypes.c_void_p, ctypes.c_int]
    _llp = ctypes.POINTER(ctypes.c_longlong)
    lib.ctcd_last_scorer_pairs.argtypes = [ctypes.c_void_p, _llp, _llp, _llp]
    lib.ctcd_stream_create_lm.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    # the blank-frame filter (blank_skip.hip): dec, x, seq_lens, B, T, V, blank_id, cmp, out_rows, out_lens, out_kept, stream
    lib.ctcd_blank_skip.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_float] + [ctypes.c_void_p] * 4
    lib.ctcd_remap_timesteps.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    lib.ctcd_remap_compact.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    lib.ctcd_remap_timesteps_host.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4
    # the blank-frame filter of live streams (stream_blank_skip.hip): dec, on, cmp_prob, cmp_log
    lib.ctcd_set_stream_blank_skip.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float]
    for name in ("ctcd_stream_frames_seen", "ctcd_stream_map_bytes"):
        getattr(lib, name).argtypes = [ctypes.c_void_p]
        getattr(lib, name).restype = ctypes.c_longlong
    lib.ctcd_last_stream_blank_skip.argtypes = [ctypes.c_void_p, _llp, _llp]
    lib.ctcd_last_stream_blank_skip_ms.argtypes = [ctypes.c_void_p, _f32p, _f32p, _f32p]
    # n-best results (nbest.hip): dec, c_hdr, c_ent, c_labels, n_labels, B, beam, T, n_best, out_tokens, out_timesteps, status, stream
    lib.ctcd_expand_compact_nbest.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_longlong] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 4
    # ... the decode entry points: `scorer`, then n_best, sit before the outputs
    lib.ctcd_beam_decode_nbest.argtypes = common[:12] + [ctypes.c_void_p, ctypes.c_int] + common[12:] + [ctypes.c_void_p]
    lib.ctcd_beam_decode_to_host_nbest.argtypes = common[:3] + [ctypes.c_int] + common[3:12] + [ctypes.c_void_p, ctypes.c_int] + common[12:] + [ctypes.c_void_p]
    # forced alignment (align.hip): dec, probs, seq_lens, B, T, V, blank_id, log_input, tokens, lens, R, L_stride, out_start, out_end,
    # out_scores, status, stream
    lib.ctcd_ctc_align.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 5
    lib.ctcd_set_align_scratch.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.ctcd_last_align_grid.argtypes = [ctypes.c_void_p]
    lib.ctcd_last_align_grid.restype = ctypes.c_longlong
    # CTC log-likelihood (loglik.hip): dec, probs, seq_lens, B, T, V, blank_id, log_input, tokens, lens, R, L_stride, out_loglik, status, stream
    lib.ctcd_ctc_loglik.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3
    lib.ctcd_set_loglik_grid.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.ctcd_last_loglik_grid.argtypes = [ctypes.c_void_p]
    lib.ctcd_last_loglik_grid.restype = ctypes.c_longlong
    # label posteriors (posterior.hip): dec, probs, seq_lens, B, T, V, blank_id, log_input, tokens, lens, R, L_stride, out_peaks,
    # out_occupancy, out_confidence, out_loglik, status, stream
    lib.ctcd_ctc_posteriors.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 6
    lib.ctcd_set_posterior_scratch.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.ctcd_last_posterior_grid.argtypes = [ctypes.c_void_p]
    lib.ctcd_last_posterior_grid.restype = ctypes.c_longlong
    # greedy decode (greedy.hip): dec, probs, seq_lens, B, T, V, blank_id, log_input, out_tokens, out_starts, out_ends, out_label_scores,
    # out_scores, out_lens, stream
    lib.ctcd_greedy_decode.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 7
    # greedy decode of live streams (greedy_stream.hip).  decode: dec, states, is_eos, probs, seq_lens, B, Tc, V, blank_id, log_input,
    # out_tokens, out_starts, out_ends, out_label_scores, out_closed_lens, out_scores, out_lens, stream
    lib.ctcd_greedy_stream_create.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_longlong]
    lib.ctcd_greedy_stream_destroy.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.ctcd_greedy_stream_destroy.restype = None
    lib.ctcd_greedy_stream_reset.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    lib.ctcd_greedy_stream_decode.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 8
    lib.ctcd_greedy_stream_info.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
    # edit distance (editdist.hip): dec, x, x_lens, B, R, L, y, y_lens, Q, Lq, out, status, stream
    lib.ctcd_edit_distance.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3
    lib.ctcd_last_edit_pairs.argtypes = [ctypes.c_void_p]
    lib.ctcd_last_edit_pairs.restype = ctypes.c_longlong
    lib.ctcd_set_edit_grid.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.ctcd_last_edit_grid.argtypes = [ctypes.c_void_p]
    lib.ctcd_last_edit_grid.restype = ctypes.c_longlong
    # edit operations (editops.hip): counts take ctcd_edit_distance's arguments; align: dec, x, x_lens, B, R, L, y, y_lens, Q, Lq, x_to_y, y_to_x, counts, status, stream
    lib.ctcd_edit_counts.argtypes = lib.ctcd_edit_distance.argtypes
    lib.ctcd_edit_align.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 5
    lib.ctcd_set_edit_scratch.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.ctcd_last_edit_slots.argtypes = [ctypes.c_void_p]
    lib.ctcd_last_edit_slots.restype = ctypes.c_longlong
    return lib


lib = _load()


class NativeError(RuntimeError):
    pass


# Destroying a scorer, a decoder or a stream frees HBM, and hipFree waits for the device.  A launch of the scorer hook that waits on
# the GPU for its answers runs the callback on the calling thread; the interpreter may collect garbage there, and a destructor run by
# that collection waited for the very launch that was waiting for the callback's answer -- until its workgroups gave up waiting, about
# six seconds later (results unchanged, one more launch).  So a destructor that runs inside a scorer callback only queues its call;
# the queue is emptied by the next checked call outside a callback (the decode that ran the callback among them).
_in_callback = 0
_deferred = []


def destroy(fn, *handles):
    """Call fn(*handles) -- a ctcd_*_destroy -- now, or after the scorer callback that is running has returned to its launch's end."""
    if _in_callback:
        _deferred.append((fn, handles))
        return
    _run_deferred()
    fn(*handles)


def _run_deferred():
    while _deferred and not _in_callback:
        fn, handles = _deferred.pop(0)
        try:
            fn(*handles)
        except Exception:
            pass


def check(rc):
    if _deferred:
        _run_deferred()
    if rc != 0:
        msg = lib.ctcd_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError("ctcdecode_amd: " + msg)
        if rc == -2:
            raise NotImplementedError("ctcdecode_amd: " + msg)
        raise NativeError("ctcdecode_amd (code %d): %s" % (rc, msg))
