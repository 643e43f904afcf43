"""MI355X-native drop-in for ``ctcdecode.CTCBeamDecoder.decode()`` (no language model).

Same constructor arguments, same ``decode(probs, seq_lens)`` call and the same four output tensors as
ctcdecode/__init__.py:6-123 of the reference; the prefix beam search itself runs as a hand-written HIP kernel
(one workgroup per utterance, beam in LDS) behind the C ABI in include/ctcdecode_amd.h.
"""
import ctypes
import inspect
import math
import operator
import weakref

import torch

from . import _native
from ._native import NativeError  # noqa: F401

__all__ = ["CTCBeamDecoder", "OnlineCTCBeamDecoder", "DecoderState", "GreedyState", "NativeError", "CallbackScorer", "KenlmScorer", "DecodePipeline", "snapshot_info"]
HAVE_LM = True  # the external-scorer tier (model_path / alpha / beta) is part of this build


class _Scorer(object):
    """ctypes owner of a ``ctcd_scorer`` (paddle_get_scorer / paddle_release_scorer, ctcdecode/__init__.py:47-50,138-140)."""

    def __init__(self, alpha, beta, model_path, labels, device_index):
        if isinstance(model_path, bytes):
            model_path = model_path.decode("utf-8")
        arr = (ctypes.c_char_p * len(labels))(*[str(x).encode("utf-8") for x in labels])
        h = ctypes.c_void_p()
        _native.check(_native.lib.ctcd_scorer_create(ctypes.byref(h), float(alpha), float(beta), str(model_path).encode("utf-8"), arr,
                                                     len(labels), int(device_index)))
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                _native.destroy(_native.lib.ctcd_scorer_destroy, h)
            except Exception:
                pass
            self.handle = None


class CallbackScorer(object):
    """The swappable scorer: a language model behind a host callback (``ctcd_scorer_create_callback``,
    include/ctcdecode_amd.h) -- the counterpart of handing the reference's decoder another ``Scorer`` implementation
    (ctcdecode/src/scorer.h:41-78).  Pass it to ``CTCBeamDecoder(..., scorer=...)`` / ``OnlineCTCBeamDecoder``.

    ``cond_log10(words)`` receives the window's ``max_order`` words (tuple of str, oldest first, ``"<s>"``-padded) and
    returns log10 p(words[-1] | words[:-1]) -- or ``None`` when the window holds a word the model does not know
    (the reference's OOV_SCORE, scorer.cpp:86-88).  It must be a pure function of the words: every distinct window is
    asked for once and cached on the device.  ``vocabulary``: the model's words (builds the dictionary of a word model;
    only single characters = character model, scorer.cpp:65-71).  An exception inside the callback fails the decode and
    is re-raised from it.
    """

    def __init__(self, cond_log10, vocabulary, max_order, labels, alpha=0.0, beta=0.0, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("ctcdecode_amd: no HIP device visible; this decoder has no CPU path")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        self._fn = cond_log10
        self._error = None

        def trampoline(_user, words, n, out):
            _native._in_callback += 1  # (a destructor that runs in here waits: _native.destroy)
            try:
                r = self._fn(tuple(words[i].decode("utf-8") for i in range(n)))
                if r is None:
                    return 1
                out[0] = float(r)
                return 0
            except BaseException as e:  # (an exception must not unwind through the C frames)
                self._error = e
                return -1
            finally:
                _native._in_callback -= 1

        self._c_fn = _native.COND_LOG10_FN(trampoline)  # kept alive with the scorer
        voc = [str(w).encode("utf-8") for w in vocabulary]
        varr = (ctypes.c_char_p * max(len(voc), 1))(*voc)
        larr = (ctypes.c_char_p * len(labels))(*[str(x).encode("utf-8") for x in labels])
        h = ctypes.c_void_p()
        _native.check(_native.lib.ctcd_scorer_create_callback(ctypes.byref(h), float(alpha), float(beta), int(max_order), varr, len(voc), self._c_fn, None,
                                                              larr, len(labels), int(index)))
        self.handle = h
        self.device_index = int(index)
        self.num_labels = len(labels)

    @classmethod
    def from_c(cls, fn_address, user_address, vocabulary, max_order, labels, alpha=0.0, beta=0.0, device=None, keepalive=None):
        """The hook with a NATIVE callback: ``fn_address`` = address of a C function of type ``ctcd_cond_log10_fn``
        (include/ctcdecode_amd.h: ``int fn(void *user, const char *const *words, int n, float *log10_prob)``), ``user_address``
        its first argument -- e.g. a thin shim over kenlm's C++ API: no Python between the decoder and the model.
        (``ctcd_scorer_cond_log10`` has this very signature: any built-in scorer can sit behind the hook -- bench.py does that to
        price the hook itself.)  ``keepalive``: objects that must outlive the scorer."""
        self = cls.__new__(cls)
        if not torch.cuda.is_available():
            raise RuntimeError("ctcdecode_amd: no HIP device visible; this decoder has no CPU path")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        self._fn, self._error, self._keepalive = None, None, keepalive
        self._c_fn = ctypes.cast(ctypes.c_void_p(int(fn_address)), _native.COND_LOG10_FN)
        voc = [str(w).encode("utf-8") for w in vocabulary]
        varr = (ctypes.c_char_p * max(len(voc), 1))(*voc)
        larr = (ctypes.c_char_p * len(labels))(*[str(x).encode("utf-8") for x in labels])
        h = ctypes.c_void_p()
        _native.check(_native.lib.ctcd_scorer_create_callback(ctypes.byref(h), float(alpha), float(beta), int(max_order), varr, len(voc), self._c_fn,
                                                              ctypes.c_void_p(int(user_address)) if user_address else None, larr, len(labels), int(index)))
        self.handle = h
        self.device_index = int(index)
        self.num_labels = len(labels)
        return self

    @classmethod
    def batched(cls, fn, vocabulary, max_order, labels, alpha=0.0, beta=0.0, device=None):
        """The hook with a BATCHED Python callback (``ctcd_scorer_create_callback_batch``): ``fn(windows)`` receives a list of
        windows -- each a tuple of ``max_order`` words, oldest first, ``"<s>"``-padded, as ``cond_log10`` receives one -- and returns a
        sequence of as many answers, each log10 p(window[-1] | window[:-1]) or ``None`` (out of vocabulary).  Same contract as the
        per-window form: a pure function of the words, every distinct window is asked once, an exception inside it (or an answer of
        the wrong length) fails the decode and is re-raised from it.  One call asks up to 512 windows: the interpreter is entered
        once per batch instead of once per window."""
        self = cls.__new__(cls)
        self._fn, self._error, self._keepalive = fn, None, None
        self._c_fn = self._batch_trampoline()  # kept alive with the scorer
        self._create_batch(vocabulary, max_order, labels, alpha, beta, device, None)
        return self

    def _batch_trampoline(self):
        def trampoline(_user, words, n, order, probs, status):
            _native._in_callback += 1  # (a destructor that runs in here waits: _native.destroy)
            try:
                flat = [w.decode("utf-8") for w in words[: n * order]]
                r = list(self._fn([tuple(flat[i * order:(i + 1) * order]) for i in range(n)]))
                if len(r) != n:
                    raise ValueError("the batched scorer callback returned %d answers for %d windows" % (len(r), n))
                for i, v in enumerate(r):
                    if v is None:
                        status[i] = 1
                    else:
                        probs[i] = float(v)
                        status[i] = 0
                return 0
            except BaseException as e:  # (an exception must not unwind through the C frames)
                self._error = e
                return -1
            finally:
                _native._in_callback -= 1

        return _native.COND_LOG10_BATCH_FN(trampoline)

    @classmethod
    def from_c_batch(cls, fn_address, user_address, vocabulary, max_order, labels, alpha=0.0, beta=0.0, device=None, keepalive=None):
        """``from_c`` for a NATIVE batched callback of type ``ctcd_cond_log10_batch_fn`` (include/ctcdecode_amd.h:
        ``int fn(void *user, const char *const *words, int n_windows, int order, float *log10_probs, int32_t *status)``).
        ``ctcd_scorer_cond_log10_batch`` has this very signature: any built-in scorer can sit behind the batched hook."""
        self = cls.__new__(cls)
        self._fn, self._error, self._keepalive = None, None, keepalive
        self._c_fn = ctypes.cast(ctypes.c_void_p(int(fn_address)), _native.COND_LOG10_BATCH_FN)
        self._create_batch(vocabulary, max_order, labels, alpha, beta, device, ctypes.c_void_p(int(user_address)) if user_address else None)
        return self

    def _create_batch(self, vocabulary, max_order, labels, alpha, beta, device, user):
        if not torch.cuda.is_available():
            raise RuntimeError("ctcdecode_amd: no HIP device visible; this decoder has no CPU path")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        voc = [str(w).encode("utf-8") for w in vocabulary]
        varr = (ctypes.c_char_p * max(len(voc), 1))(*voc)
        larr = (ctypes.c_char_p * len(labels))(*[str(x).encode("utf-8") for x in labels])
        h = ctypes.c_void_p()
        _native.check(_native.lib.ctcd_scorer_create_callback_batch(ctypes.byref(h), float(alpha), float(beta), int(max_order), varr, len(voc), self._c_fn,
                                                                    user, larr, len(labels), int(index)))
        self.handle = h
        self.device_index = int(index)
        self.num_labels = len(labels)

    def callback_calls(self):
        """Distinct windows the callback has been asked for so far."""
        return int(_native.lib.ctcd_scorer_callback_calls(self.handle))

    def callback_batches(self):
        """Calls of a batched callback so far (``batched`` / ``from_c_batch``; 0 for the per-window form)."""
        return int(_native.lib.ctcd_scorer_callback_batches(self.handle))

    def callback_seconds(self):
        """Time spent inside the callback so far (an estimate: every 16th call is timed)."""
        return float(_native.lib.ctcd_scorer_callback_seconds(self.handle))

    def set_callback_threads(self, threads):
        """A NATIVE callback that may be called from several threads at once (``from_c`` over a read-only model): ``threads - 1``
        helper threads ask beside the calling one while a launch waits for its answers (``ctcd_scorer_set_callback_threads``).
        Refused for Python callables: the interpreter lock would serialise them; a batched callback takes no helper threads either."""
        if self._fn is not None and int(threads) != 1:
            raise ValueError("callback threads are for native callbacks (CallbackScorer.from_c): a Python callable runs under the interpreter lock")
        _native.check(_native.lib.ctcd_scorer_set_callback_threads(self.handle, int(threads)))

    def _raise_pending(self):
        e, self._error = self._error, None
        if e is not None:
            raise e

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                _native.destroy(_native.lib.ctcd_scorer_destroy, h)
            except Exception:
                pass
            self.handle = None


class KenlmScorer(CallbackScorer):
    """A kenlm model -- binary files included -- behind the scorer hook, through the ``kenlm`` Python module (not part of
    this image: ImportError if it is missing).  ``vocabulary``: the model's words (a binary model does not list them; pass
    the word list it was trained with, as the reference's Scorer reads them from the model, scorer.cpp:196-230).  The model is
    asked through the batched hook (``CallbackScorer.batched``): one call per batch of windows, each window scored as before."""

    def __init__(self, model_path, vocabulary, labels, alpha=0.0, beta=0.0, device=None):
        import kenlm  # noqa: F401  (optional dependency)

        self._model = kenlm.Model(str(model_path))
        model = self._model
        self._fn, self._error, self._keepalive = (lambda windows: [KenlmScorer.cond_log10(kenlm, model, w) for w in windows]), None, None
        self._c_fn = self._batch_trampoline()
        self._create_batch(vocabulary, model.order, labels, alpha, beta, device, None)

    @staticmethod
    def cond_log10(kenlm, model, words):
        """One window through a kenlm ``model`` (``kenlm``: the module): Scorer::get_log_cond_prob (scorer.cpp:74-93) -- the window
        is fed from the empty context, None (out of vocabulary) if any word is unknown, else the last word's BaseScore."""
        state, out = kenlm.State(), kenlm.State()
        model.NullContextWrite(state)
        p = 0.0
        for w in words:
            if w not in model:
                return None
            p = model.BaseScore(state, w, out)
            state, out = out, state
        return p


# include/ctcdecode_amd.h CTCD_DTYPE_*: device tensors of these dtypes go to the library as they are (its kernels widen them)
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2
_LAUNCH_ORDERS = {"batch": 0, "length": 1}  # include/ctcdecode_amd.h CTCD_ORDER_BATCH / CTCD_ORDER_LENGTH
_HALF_DTYPES = {torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16}


def _input_rows(owner, probs):
    """``probs`` as the library reads it: on the owner's device and contiguous; a HIP tensor of dtype float16 / bfloat16 keeps its
    dtype -- the decoder reads half rows itself, exactly as it would read their float32 copy, and no copy is made -- and every other
    tensor becomes float32, as in the reference.  Sets the decoder's input dtype for the call (``ctcd_set_input_dtype``): it is state
    of the decoder object, so threads that share one decoder and pass different dtypes must not interleave their calls."""
    code = _HALF_DTYPES.get(probs.dtype, DTYPE_F32) if probs.is_cuda else DTYPE_F32
    probs = probs.to(device=owner._device, dtype=probs.dtype if code else torch.float32).contiguous()
    _set_input_dtype(owner, code)
    return probs


def _set_input_dtype(owner, code):
    if getattr(owner, "_in_dtype", DTYPE_F32) != code:
        _native.check(_native.lib.ctcd_set_input_dtype(owner._handle, code))
        owner._in_dtype = code


def _to_host(tensors):
    """Device -> host copy of the result tensors through page-locked memory (PyTorch's caching host allocator recycles
    the blocks), all copies in flight together, one synchronisation: several times faster than ``.cpu()`` on pageable
    memory for the 2 x [B, K, T] int32 results."""
    outs = []
    for t in tensors:
        h = torch.empty(t.shape, dtype=t.dtype, device="cpu", pin_memory=True)
        h.copy_(t, non_blocking=True)
        outs.append(h)
    torch.cuda.current_stream(tensors[0].device).synchronize()
    return tuple(outs)


def _last_scorer_pairs(handle):
    q, d, r = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_longlong()
    _native.check(_native.lib.ctcd_last_scorer_pairs(handle, ctypes.byref(q), ctypes.byref(d), ctypes.byref(r)))
    return int(q.value), int(d.value), int(r.value)


def _last_kernel(handle):
    if not handle:  # (a ctypes.c_void_p holding NULL is false; the C call answers -1 both for "no launch yet" and for a NULL decoder)
        raise ValueError("ctcdecode_amd: the decoder has no native handle")
    out = (ctypes.c_int32 * 7)()
    rc = _native.lib.ctcd_debug_last_kernel(handle, out)
    if rc == -1:
        return None
    _native.check(rc)
    return tuple(int(v) for v in out)


# include/ctcdecode_amd.h CTCD_PP_*: the pre-pass kernels, and the stages ctcd_debug_last_prepass reports them in
PREPASS_KERNELS = {1: "prob_to_log", 2: "widen", 3: "lsm_wave", 4: "lsm_wg", 5: "prune_rows", 6: "prune_wg", 7: "prune_logits", 8: "resolve"}
PREPASS_STAGES = ("elementwise", "log_softmax", "prune", "resolve")
DTYPE_NAMES = {DTYPE_F32: "f32", DTYPE_F16: "f16", DTYPE_BF16: "bf16"}


def _last_prepass(handle):
    if not handle:
        raise ValueError("ctcdecode_amd: the decoder has no native handle")
    out = (ctypes.c_int32 * 16)()
    _native.check(_native.lib.ctcd_debug_last_prepass(handle, out))
    return {st: (PREPASS_KERNELS[out[4 * i]], int(out[4 * i + 1]), int(out[4 * i + 2]), DTYPE_NAMES[out[4 * i + 3]]) if out[4 * i] else None
            for i, st in enumerate(PREPASS_STAGES)}


def prepass_table():
    """Every pre-pass kernel instantiation of the build (include/ctcdecode_amd.h ctcd_debug_prepass_table): a list of
    (kernel, a, b, dtype, largest V the dispatch sends to it or 0), named as ``last_prepass()`` names them."""
    n = int(_native.lib.ctcd_debug_prepass_table(None, 0))
    out = (ctypes.c_int32 * (5 * n))()
    _native.lib.ctcd_debug_prepass_table(out, n)
    return [(PREPASS_KERNELS[out[5 * i]], int(out[5 * i + 1]), int(out[5 * i + 2]), DTYPE_NAMES[out[5 * i + 3]], int(out[5 * i + 4]))
            for i in range(n)]


def _adopt_scorer(scorer, model_path, num_labels, device_index):
    if model_path:
        raise ValueError("pass either model_path or scorer, not both")
    if not isinstance(scorer, CallbackScorer):
        raise TypeError("scorer must be a ctcdecode_amd.CallbackScorer (or KenlmScorer)")
    if scorer.num_labels != num_labels or scorer.device_index != device_index:
        raise ValueError("the scorer was built for other labels / another device than this decoder")
    return scorer


def _blank_skip_threshold(thr):
    """The constructor's ``blank_skip``: None (off) or a float in (0, 1]."""
    if thr is None:
        return None
    if isinstance(thr, bool) or not isinstance(thr, (int, float)):
        raise ValueError("blank_skip must be None or a float in (0, 1], not %r" % (thr,))
    thr = float(thr)
    if not (0.0 < thr <= 1.0):  # (NaN fails both compares)
        raise ValueError("blank_skip must be None or a float in (0, 1], not %r" % (thr,))
    return thr


def _f32(x):
    """``x`` rounded to float32 (numpy.float32(x)), as a Python float."""
    return ctypes.c_float(x).value


def _n_best(n_best, beam_width):
    """A one-shot call's ``n_best``: None (every row, today's path) or an integer in [1, beam_width]."""
    if n_best is None:
        return None
    if isinstance(n_best, bool) or isinstance(n_best, float):
        raise ValueError("n_best must be None or an integer in [1, beam_width], not %r" % (n_best,))
    try:
        n = operator.index(n_best)
    except TypeError:
        raise ValueError("n_best must be None or an integer in [1, beam_width], not %r" % (n_best,))
    if not 1 <= n <= int(beam_width):
        raise ValueError("n_best must be None or an integer in [1, beam_width = %d], not %r" % (int(beam_width), n_best))
    return n


class CTCBeamDecoder(object):
    """See ctcdecode/__init__.py:6-51 of the reference for the meaning of the arguments.

    Differences, all additive:
      * ``device``: the MI355X to decode on (default: ``cuda:<current>``).
      * ``decode_device()`` returns the four tensors in HBM without the device->host copy.
      * positions the reference leaves uninitialised (``[b, p, out_len:]``, rows ``p >= #results``) are zero.
      * ``model_path`` must be an ARPA text model (binary kenlm files are not supported); the scorer's tables are mirrored
        into HBM and queried inside the decode kernel (include/ctcdecode_amd.h, "LM tier").
      * ``n_best`` on every one-shot call (``decode``, ``decode_device``, ``decode_padded``, ``expand_compact``,
        ``DecodePipeline.submit``): None (default) returns all ``beam_width`` rows as ever; an integer n in [1, beam_width] returns
        rows 0 .. n-1 alone -- ``output`` / ``timesteps`` [B, n, T], ``scores`` / ``out_lens`` [B, n] -- equal to the full call's
        ``[:, :n]`` and zero wherever the full call defines nothing (include/ctcdecode_amd.h "n-best results").
      * ``blank_skip``: None (default, off) or a threshold in (0, 1]: every one-shot call drops, on the device and before the beam
        search, the frames whose blank posterior is GREATER than the threshold, decodes the kept frames, and reports time steps
        as original frame numbers (include/ctcdecode_amd.h "Blank-frame filter").  The outputs keep their [B, K, T] shapes.
        The results are those of the reference on the kept frames -- not those of the full decode: a repeated label whose
        separating blank frames are all skipped collapses.  ``OnlineCTCBeamDecoder`` has it as ``set_blank_skip(thr)``.
    """

    def __init__(self, labels, model_path=None, alpha=0, beta=0, cutoff_top_n=40, cutoff_prob=1.0, beam_width=100,
                 num_processes=4, blank_id=0, log_probs_input=False, device=None, logits_input=False, scorer=None, blank_skip=None):
        self._blank_skip = _blank_skip_threshold(blank_skip)
        self._last_skip = None
        self.cutoff_top_n = cutoff_top_n
        self._beam_width = beam_width
        self._scorer = None
        self._num_processes = num_processes
        self._labels = list(labels)
        self._num_labels = len(labels)
        self._blank_id = blank_id
        # logits_input (extension, not in the reference): the input holds raw logits; the device normalises them with a
        # float32 log_softmax (include/ctcdecode_amd.h ctcd_log_softmax) before decoding
        self._log_probs = 2 if logits_input else (1 if log_probs_input else 0)
        self._cutoff_prob = cutoff_prob
        if not torch.cuda.is_available():
            raise RuntimeError("ctcdecode_amd: no HIP device visible; this decoder has no CPU path")
        self._device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self._device.type != "cuda":
            raise ValueError("ctcdecode_amd: device must be a HIP (cuda:N) device")
        if self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        h = ctypes.c_void_p()
        _native.check(_native.lib.ctcd_create(ctypes.byref(h), self._device.index))
        self._handle = h
        if scorer is not None:  # a ready-made scorer object (CallbackScorer / KenlmScorer): the swappable-scorer hook
            self._scorer = _adopt_scorer(scorer, model_path, self._num_labels, self._device.index)
        elif model_path:  # ctcdecode/__init__.py:47-50 (`if model_path:`: None and "" both mean no scorer)
            self._scorer = _Scorer(alpha, beta, model_path, self._labels, self._device.index)

    def _check(self, rc):
        """``_native.check`` for the calls a scorer callback runs under: an exception raised inside the callback comes first."""
        if rc and self._scorer is not None and hasattr(self._scorer, "_raise_pending"):
            self._scorer._raise_pending()
        _native.check(rc)

    def set_threads(self, n):
        _native.check(_native.lib.ctcd_set_threads(self._handle, int(n)))

    def set_launch_order(self, order="batch"):
        """"length": the workgroups of a launch take their utterances longest first (ranked by ``seq_lens`` on the device), so that a
        long utterance of a batch larger than the device's resident workgroups does not start last and run on alone; "batch"
        (default): workgroup i decodes utterance i.  Results are bit-identical either way (include/ctcdecode_amd.h
        ctcd_set_launch_order).  Applies to every one-shot call (not to OnlineCTCBeamDecoder)."""
        if order not in _LAUNCH_ORDERS:
            raise ValueError("launch order must be 'batch' or 'length', not %r" % (order,))
        _native.check(_native.lib.ctcd_set_launch_order(self._handle, _LAUNCH_ORDERS[order]))

    def last_launch_order(self):
        """The permutation the last call's workgroups took their utterances in (numpy int32 [B]: rank -> utterance), or None if that
        call ran in batch order.  Waits for that call's order pass."""
        import numpy as np

        B = getattr(self, "_last_batch", 0)
        out = np.empty((max(B, 1),), np.int32)
        rc = _native.lib.ctcd_debug_last_launch_order(self._handle, out.ctypes.data_as(_native._i32p), B)
        if rc < 0:
            _native.check(rc)
        return out[:B] if rc == 1 else None

    def set_cu_sharing(self, mode=1):
        """1: always launch the two-workgroups-per-CU build of the kernel (beam <= 128, <= 32 labels) -- for a serving loop
        that keeps several launches in flight; 0: never; -1 (default): when a batch has more utterances than the GPU has CUs."""
        _native.check(_native.lib.ctcd_set_cu_sharing(self._handle, int(mode)))

    def set_exact_shape(self, mode=-1):
        """Exact-shape kernels (include/ctcdecode_amd.h ctcd_set_exact_shape): builds of the plain north-star kernel with beam width,
        label count and blank index as constants -- beam 100 over 29 labels, blank 0.  -1 (default): wherever a call has exactly that
        shape; 0: never; 1: required (a call that does not qualify raises and launches nothing).  Results are bit-identical."""
        _native.check(_native.lib.ctcd_set_exact_shape(self._handle, int(mode)))

    def last_exact_shape(self):
        """1 if the last launch ran an exact-shape kernel, else 0."""
        return int(_native.lib.ctcd_last_exact_shape(self._handle))

    def set_subtree_search(self, mode=-1):
        """Phase A1's four-subtrees-per-wave build of the north-star class kernel (include/ctcdecode_amd.h): -1 = chosen from the beam
        shape the last checked launch reported (chain-shaped beams, i.e. blank-dominated rows: on), 0 / 1 = never / always."""
        _native.check(_native.lib.ctcd_set_subtree_search(self._handle, int(mode)))

    def last_subtree_search(self):
        return int(_native.lib.ctcd_last_subtree_search(self._handle))

    def last_layout(self):
        """Test hook: the workspace layout of the last launch's kernel (include/ctcdecode_amd.h ctcd_debug_last_layout): 0 run-time,
        1 fixed (beam <= 128, <= 32 labels), 2 the pruned default's (beam <= 112, cutoff_top_n <= 40), 3 wide beams at a compile-time
        size, 4-6 wide beams with HBM scratch; -1 none yet."""
        return int(_native.lib.ctcd_debug_last_layout(self._handle))

    def last_kernel(self):
        """Test hook: the template arguments (PROF, BIG, LAYOUT, PRUNED, NT, LM, OCC2) of the kernel instantiation the last launch used
        (include/ctcdecode_amd.h ctcd_debug_last_kernel), or None before any launch."""
        return _last_kernel(self._handle)

    def last_prepass(self):
        """Test hook: the pre-pass kernels the last call launched (include/ctcdecode_amd.h ctcd_debug_last_prepass), as a dict over the
        stages "elementwise", "log_softmax", "prune", "resolve" of None (nothing launched) or (kernel, a, b, dtype): kernel one of
        "prob_to_log", "widen", "lsm_wave", "lsm_wg" (a = F4), "prune_rows" (a = R), "prune_wg" (a = F4, b = REG), "prune_logits" (a = F4),
        "resolve" (b = 1: its arrays in global memory); dtype "f32" / "f16" / "bf16"."""
        return _last_prepass(self._handle)

    def set_host_path(self, input_streaming=None, mirror_cap_labels=None):
        """Test hook for decode(): turn the streamed input off / on; shrink the host mirror of the compact results."""
        _native.check(_native.lib.ctcd_debug_set_host_path(self._handle, -1 if input_streaming is None else int(bool(input_streaming)),
                                                           -2 if mirror_cap_labels is None else int(mirror_cap_labels)))

    def set_fixed_layout(self, on=True):
        """Test hook: False forces the run-time workspace layout also for small shapes (identical results)."""
        _native.check(_native.lib.ctcd_debug_set_fixed_layout(self._handle, 1 if on else 0))

    def set_scorer_wait(self, on=True):
        """Callback scorers: True (default) = a launch waits on the GPU for the callback's answers; False = every miss ends the
        utterance's launch and the host relaunches (the form of rounds 4-5).  Identical results."""
        _native.check(_native.lib.ctcd_set_scorer_wait(self._handle, 1 if on else 0))

    def last_scorer_launches(self):
        """(launches, answer batches handed to waiting launches) of the last decode with a callback scorer."""
        return int(_native.lib.ctcd_last_scorer_rounds(self._handle)), int(_native.lib.ctcd_last_scorer_waits(self._handle))

    def set_scorer_filter(self, on=True):
        """Callback scorers: True (default) = the kernels drop a parked utterance's repeated misses on one (history, word) pair;
        False = every miss is queued (measurements and tests: identical results, more queued pairs)."""
        _native.check(_native.lib.ctcd_set_scorer_filter(self._handle, 1 if on else 0))

    def last_scorer_pairs(self):
        """(queued pairs, windows asked, repeats by the same item) of the last decode with a callback scorer
        (include/ctcdecode_amd.h ctcd_last_scorer_pairs)."""
        return _last_scorer_pairs(self._handle)

    def set_fused_logits(self, on=True):
        """Test hook (logits_input=True): False sends raw logits through the one-wave log_softmax pass and the separate prune
        instead of the workgroup kernels / the fused logits-to-candidates pass (identical results)."""
        _native.check(_native.lib.ctcd_debug_set_fused_logits(self._handle, 1 if on else 0))

    def set_prune_registers(self, on=True):
        """Test hook: False makes the workgroup prune pass read every row twice (the form of rounds 2-5) instead of keeping it in
        registers (identical results)."""
        _native.check(_native.lib.ctcd_debug_set_prune_registers(self._handle, 1 if on else 0))

    def last_prune_rows(self, rows, stride):
        """Test hook: the vocabulary-prune pass's output of the last call as numpy arrays (counts[rows], labels and values
        [rows, stride], stride = min(cutoff_top_n, V); entries at or beyond a frame's count are unspecified)."""
        import numpy as np

        cnt = np.zeros((rows,), np.int32)
        lab = np.zeros((rows, stride), np.int32)
        val = np.zeros((rows, stride), np.float32)
        _native.check(_native.lib.ctcd_debug_prune_rows(self._handle, rows, stride, cnt.ctypes.data, lab.ctypes.data, val.ctypes.data))
        return cnt, lab, val

    def set_timing(self, on=True):
        _native.check(_native.lib.ctcd_set_timing(self._handle, 1 if on else 0))

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        _native.check(_native.lib.ctcd_last_kernel_ms(self._handle, ctypes.byref(ms)))
        return float(ms.value)

    def last_prune_ms(self):
        ms = ctypes.c_float()
        _native.check(_native.lib.ctcd_last_prune_ms(self._handle, ctypes.byref(ms)))
        return float(ms.value)

    def last_resolve_ms(self):
        """(set_timing) the flagged frames' replay behind the prune pass of the last call: from the end of the prune pass to the
        start of the decode kernel."""
        ms = ctypes.c_float()
        _native.check(_native.lib.ctcd_last_resolve_ms(self._handle, ctypes.byref(ms)))
        return float(ms.value)

    def _skip_rows(self, probs, seq_lens):
        """The blank-frame filter in front of a one-shot call.  ``probs``: the call's rows as ``_input_rows`` returned them, ``seq_lens``
        on the device or None.  -> (rows, seq_lens', kept, log mode the decode is to be told), or None when the filter is off or there
        is nothing to filter.  Everything is queued on the current stream; the temporaries are torch allocations there.  Raw logits
        go through the log-softmax pass first (float32), are filtered in log mode, and the decode is told log-probabilities."""
        B, T, V = probs.shape
        if self._blank_skip is None:
            return None
        if B == 0 or T == 0:
            self._last_skip = (None, None, 0, 0)
            return None
        if not 0 <= int(self._blank_id) < V:
            raise ValueError("ctcdecode_amd: blank_id must index the vocabulary")
        mode = self._log_probs
        cmp = _f32(self._blank_skip) if mode == 0 else _f32(math.log(self._blank_skip))
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            lens_ptr = seq_lens.data_ptr() if seq_lens is not None else None
            if mode == 2:
                lsm = torch.empty((B, T, V), dtype=torch.float32, device=self._device)  # (frames beyond seq_lens: never read)
                _native.check(_native.lib.ctcd_log_softmax(self._handle, probs.data_ptr(), lens_ptr, B, T, V, lsm.data_ptr(), stream))
                probs, mode = lsm, 1
                _set_input_dtype(self, DTYPE_F32)
            rows = torch.empty_like(probs)
            kept = torch.empty((B, T), dtype=torch.int32, device=self._device)
            lens = torch.empty((B,), dtype=torch.int32, device=self._device)
            _native.check(_native.lib.ctcd_blank_skip(self._handle, probs.data_ptr(), lens_ptr, B, T, V, int(self._blank_id), cmp,
                                                      rows.data_ptr(), lens.data_ptr(), kept.data_ptr(), stream))
        self._last_skip = (seq_lens, lens, B, T)
        return rows, lens, kept, mode

    def skip_blank_frames(self, probs, seq_lens=None):
        """The filter ``blank_skip`` puts in front of every one-shot call, on its own (the counterpart of ``log_softmax``): returns
        (rows [B, T, V], seq_lens' [B], kept [B, T]) in HBM -- rows ``[b, :seq_lens'[b]]`` are the kept frames of utterance b in order
        (the rest is unspecified), ``kept[b, i]`` the original index of the i-th of them (0 from ``seq_lens'[b]`` on).  Follows the
        decoder's ``blank_id`` and input mode; with ``logits_input=True`` the rows are those of ``log_softmax`` (float32), otherwise
        they keep the dtype ``decode_device`` would read."""
        if self._blank_skip is None:
            raise ValueError("skip_blank_frames needs a decoder built with blank_skip")
        if probs.dim() != 3:
            raise ValueError("probs must be [batch, time, labels]")
        probs = _input_rows(self, probs)
        B, T, V = probs.shape
        if seq_lens is not None:
            seq_lens = seq_lens.to(device=self._device, dtype=torch.int32).contiguous()
            if seq_lens.numel() != B:
                raise ValueError("seq_lens must have one entry per batch item")
        sk = self._skip_rows(probs, seq_lens)
        if sk is None:  # no utterance or no frame
            return (probs, torch.zeros((B,), dtype=torch.int32, device=self._device), torch.zeros((B, T), dtype=torch.int32, device=self._device))
        return sk[0], sk[1], sk[2]

    def last_blank_skip(self):
        """Test hook: (frames considered, frames kept) of the last call's filter, or None if no call has filtered yet.  Waits for
        that call."""
        st = self._last_skip
        if st is None:
            return None
        lens, kept_lens, B, T = st
        if kept_lens is None:
            return 0, 0
        considered = B * T if lens is None else int(lens.clamp(0, T).sum().item())
        return considered, int(kept_lens.sum().item())

    def decode_device(self, probs, seq_lens=None, check=True, n_best=None):
        """``probs``: [B, T, V] tensor (any device / float dtype).  Returns (beam_results, beam_scores, timesteps,
        out_lens) as tensors in HBM on the decoder's device; asynchronous on the current stream when ``check`` is False.
        A HIP tensor of dtype bfloat16 / float16 is decoded as it is, without a float32 copy: the results are those of
        ``probs.float()``, bit for bit.  Other dtypes are cast to float32 first.  ``n_best``: rows 0 .. n-1 alone (see the class)."""
        if probs.dim() != 3:
            raise ValueError("probs must be [batch, time, labels]")
        n_best = _n_best(n_best, self._beam_width)
        probs = _input_rows(self, probs)
        B, T, V = probs.shape
        if V != self._num_labels:
            raise ValueError("probs.shape[2] (%d) does not match the number of labels (%d)" % (V, self._num_labels))
        if seq_lens is not None:
            seq_lens = seq_lens.to(device=self._device, dtype=torch.int32).contiguous()
            if seq_lens.numel() != B:
                raise ValueError("seq_lens must have one entry per batch item")
        K = self._beam_width
        log_mode, kept = self._log_probs, None
        sk = self._skip_rows(probs, seq_lens)
        if sk is not None:  # blank_skip: the decode sees the kept rows and their counts
            probs, seq_lens, kept, log_mode = sk
        R = K if n_best is None else n_best  # result rows per item
        with torch.cuda.device(self._device):
            output = torch.empty((B, R, T), dtype=torch.int32, device=self._device)
            timesteps = torch.empty((B, R, T), dtype=torch.int32, device=self._device)
            scores = torch.empty((B, R), dtype=torch.float32, device=self._device)
            out_len = torch.empty((B, R), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            if n_best is not None:  # compact records into the decoder's scratch, the n-best expansion behind them on the stream
                self._check(_native.lib.ctcd_beam_decode_nbest(
                    self._handle, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, B, T, V, K,
                    self._num_processes, float(self._cutoff_prob), int(self.cutoff_top_n), int(self._blank_id), log_mode,
                    self._scorer.handle if self._scorer is not None else None, n_best, output.data_ptr(), timesteps.data_ptr(),
                    scores.data_ptr(), out_len.data_ptr(), None, stream))
                self._last_batch = B  # (last_launch_order: the batch of the last call that was queued)
            elif self._scorer is not None:  # ctcdecode/__init__.py:87-104 (paddle_beam_decode_lm)
                self._check(_native.lib.ctcd_beam_decode_lm(
                    self._handle, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, B, T, V, K,
                    self._num_processes, float(self._cutoff_prob), int(self.cutoff_top_n), int(self._blank_id), log_mode,
                    self._scorer.handle, output.data_ptr(), timesteps.data_ptr(), scores.data_ptr(), out_len.data_ptr(), None, stream))
                self._last_batch = B  # (last_launch_order: the batch of the last call that was queued)
            else:
                _native.check(_native.lib.ctcd_beam_decode(
                    self._handle, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, B, T, V, K,
                    self._num_processes, float(self._cutoff_prob), int(self.cutoff_top_n), int(self._blank_id), log_mode,
                    output.data_ptr(), timesteps.data_ptr(), scores.data_ptr(), out_len.data_ptr(), None, stream))
                self._last_batch = B  # (last_launch_order: the batch of the last call that was queued)
            if kept is not None and K > 0:  # time steps back to original frame numbers, behind the decode on its stream
                _native.check(_native.lib.ctcd_remap_timesteps(self._handle, timesteps.data_ptr(), out_len.data_ptr(), kept.data_ptr(),
                                                               seq_lens.data_ptr(), B, R, T, stream))
            if check:
                _native.check(_native.lib.ctcd_check_status(self._handle, B))
        return output, scores, timesteps, out_len

    def decode(self, probs, seq_lens=None, *, n_best=None):
        """Drop-in for ctcdecode/__init__.py:53-123: returns CPU tensors (output, scores, timesteps, out_seq_len).

        The results leave the GPU in compact form (every beam only the labels it does not share with its neighbour in the
        trie, include/ctcdecode_amd.h) and ``num_processes`` host threads expand them into the four tensors.

        A HIP tensor of dtype bfloat16 / float16 is decoded without a float32 copy (the results of ``probs.float()``, bit for
        bit); a CPU tensor of any dtype is cast to float32 on the host, as the reference does (ctcdecode/__init__.py:77).

        ``n_best``: rows 0 .. n-1 alone (see the class): the page-locked tensors are [B, n, T] and the host threads expand those rows only."""
        if probs.dim() != 3:
            raise ValueError("probs must be [batch, time, labels]")
        n_best = _n_best(n_best, self._beam_width)
        on_dev = probs.is_cuda
        if on_dev:
            probs = _input_rows(self, probs)
        else:
            probs = probs.to(dtype=torch.float32).contiguous()  # ctcdecode/__init__.py:77
            _set_input_dtype(self, DTYPE_F32)
        B, T, V = probs.shape
        if V != self._num_labels:
            raise ValueError("probs.shape[2] (%d) does not match the number of labels (%d)" % (V, self._num_labels))
        if seq_lens is not None:
            seq_lens = seq_lens.to(device=self._device if on_dev else "cpu", dtype=torch.int32).contiguous()
            if seq_lens.numel() != B:
                raise ValueError("seq_lens must have one entry per batch item")
        K = self._beam_width
        log_mode, kept_host = self._log_probs, None
        if self._blank_skip is not None and B > 0 and T > 0:
            # blank_skip: a CPU input is uploaded whole (it is not streamed in on this route), the filter runs on the device, and the
            # map and the counts start their way to page-locked memory while the decode runs
            if not on_dev:
                probs = probs.to(device=self._device)
                if seq_lens is not None:
                    seq_lens = seq_lens.to(device=self._device)
                on_dev = True
            probs, seq_lens, kept, log_mode = self._skip_rows(probs, seq_lens)
            with torch.cuda.device(self._device):
                kept_host = (torch.empty((B, T), dtype=torch.int32, pin_memory=True), torch.empty((B,), dtype=torch.int32, pin_memory=True))
                kept_host[0].copy_(kept, non_blocking=True)
                kept_host[1].copy_(seq_lens, non_blocking=True)
        elif self._blank_skip is not None:
            self._last_skip = (None, None, 0, 0)
        R = K if n_best is None else n_best  # result rows per item
        pin = B * R * T > 0
        output = torch.empty((B, R, T), dtype=torch.int32, pin_memory=pin)
        timesteps = torch.empty((B, R, T), dtype=torch.int32, pin_memory=pin)
        scores = torch.empty((B, R), dtype=torch.float32, pin_memory=pin)
        out_len = torch.empty((B, R), dtype=torch.int32, pin_memory=pin)
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            if n_best is not None:
                self._check(_native.lib.ctcd_beam_decode_to_host_nbest(
                    self._handle, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, 1 if on_dev else 0, B, T, V, K,
                    self._num_processes, float(self._cutoff_prob), int(self.cutoff_top_n), int(self._blank_id), log_mode,
                    self._scorer.handle if self._scorer is not None else None, n_best, output.data_ptr(), timesteps.data_ptr(),
                    scores.data_ptr(), out_len.data_ptr(), None, stream))
            else:
                self._check(_native.lib.ctcd_beam_decode_to_host(
                    self._handle, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, 1 if on_dev else 0, B, T, V, K,
                    self._num_processes, float(self._cutoff_prob), int(self.cutoff_top_n), int(self._blank_id), log_mode,
                    self._scorer.handle if self._scorer is not None else None, output.data_ptr(), timesteps.data_ptr(), scores.data_ptr(),
                    out_len.data_ptr(), None, stream))
            self._last_batch = B  # (last_launch_order: the batch of the last call that was queued)
            if kept_host is not None and K > 0:
                # the map applied on the host, to the valid prefixes alone -- no second pass over the padded tensors -- by as many threads
                # as the native call expands the results with (max(num_processes, 16))
                torch.cuda.current_stream(self._device).synchronize()
                _native.check(_native.lib.ctcd_remap_timesteps_host(timesteps.data_ptr(), out_len.data_ptr(), kept_host[0].data_ptr(),
                                                                    kept_host[1].data_ptr(), B, R, T, max(int(self._num_processes), 16)))
        return output, scores, timesteps, out_len

    # The drop-in call declares the reference's parameters and nothing else (ctcdecode/__init__.py:53; tests/test_abi.py holds the class
    # to it): code that inspects ``decode`` sees ``(self, probs, seq_lens=None)``.  ``n_best`` is an extension that can only be given by
    # keyword; it is documented in the docstring above and in the class's.
    decode.__signature__ = inspect.Signature([inspect.Parameter("self", inspect.Parameter.POSITIONAL_OR_KEYWORD),
                                              inspect.Parameter("probs", inspect.Parameter.POSITIONAL_OR_KEYWORD),
                                              inspect.Parameter("seq_lens", inspect.Parameter.POSITIONAL_OR_KEYWORD, default=None)])

    def log_softmax(self, logits, seq_lens=None):
        """The float32 log_softmax that ``logits_input=True`` applies before decoding, as a tensor in HBM ([B, T, V]; frames at
        or beyond ``seq_lens`` are left 0).  Bit-reproducible: see include/ctcdecode_amd.h ctcd_log_softmax.  bfloat16 / float16
        logits on the device are read as they are (the result is that of ``logits.float()``); the output is float32."""
        if logits.dim() != 3:
            raise ValueError("logits must be [batch, time, labels]")
        logits = _input_rows(self, logits)
        B, T, V = logits.shape
        if seq_lens is not None:
            seq_lens = seq_lens.to(device=self._device, dtype=torch.int32).contiguous()
        with torch.cuda.device(self._device):
            out = torch.zeros((B, T, V), dtype=torch.float32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(_native.lib.ctcd_log_softmax(self._handle, logits.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None,
                                                       B, T, V, out.data_ptr(), stream))
        return out

    def _score_rows(self, name, entry, probs, seq_lens, beam_results, out_lens, outputs):
        """What ``align``, ``log_likelihood`` and ``label_posteriors`` (``name``, for the error text) share: the shape checks, the tensors
        moved to the device, the call of ``entry`` (ctcd_ctc_align / ctcd_ctc_loglik / ctcd_ctc_posteriors) and the status read.  ``outputs``: (one value per label?, dtype) for each
        output tensor of the entry point.  -> the output tensors, [B, R, L] or [B, R], on the device."""
        if probs.dim() != 3:
            raise ValueError("probs must be [batch, time, labels]")
        if beam_results.dim() != 3 or out_lens.dim() != 2 or tuple(out_lens.shape) != tuple(beam_results.shape[:2]):
            raise ValueError("beam_results must be [batch, rows, labels] and out_lens [batch, rows]")
        probs = _input_rows(self, probs)
        B, T, V = probs.shape
        if beam_results.shape[0] != B:
            raise ValueError("beam_results.shape[0] (%d) does not match the batch (%d)" % (beam_results.shape[0], B))
        if V != self._num_labels:
            raise ValueError("probs.shape[2] (%d) does not match the number of labels (%d)" % (V, self._num_labels))
        if not 0 <= int(self._blank_id) < V:
            raise ValueError("ctcdecode_amd: blank_id must index the vocabulary")
        if seq_lens is not None:
            seq_lens = seq_lens.to(device=self._device, dtype=torch.int32).contiguous()
            if seq_lens.numel() != B:
                raise ValueError("seq_lens must have one entry per batch item")
        tokens = beam_results.to(device=self._device, dtype=torch.int32).contiguous()
        lens = out_lens.to(device=self._device, dtype=torch.int32).contiguous()
        R, L = int(tokens.shape[1]), int(tokens.shape[2])
        with torch.cuda.device(self._device):
            outs = [torch.empty((B, R, L) if per_label else (B, R), dtype=dtype, device=self._device) for per_label, dtype in outputs]
            status = torch.zeros((max(B, 1),), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(entry(self._handle, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, B, T, V, int(self._blank_id),
                                self._log_probs, tokens.data_ptr(), lens.data_ptr(), R, L, *[o.data_ptr() for o in outs], status.data_ptr(), stream))
            bad = torch.nonzero(status[:B]).flatten().tolist() if B else []
        if bad:
            raise ValueError("ctcdecode_amd: %s: items %s have a row with a label outside the vocabulary, a blank label or a length outside "
                             "[0, %d] (CTCD_ALIGN_BAD_ROW)" % (name, bad[:8], L))
        return outs

    def align(self, probs, seq_lens, beam_results, out_lens):
        """CTC forced alignment on the device (include/ctcdecode_amd.h "Forced alignment"): for every row ``beam_results[b, r, :out_lens[b, r]]``
        the best path of its labels through the rows ``probs[b, :seq_lens[b]]``.  Returns ``(starts, ends, scores)``: ``starts`` / ``ends``
        int32 [B, R, L], the first and last frame (inclusive) each label occupies, 0 at or beyond a row's length; ``scores`` float32
        [B, R], the path's log-probability -- a Viterbi score that does not depend on what the beam search pruned (``timesteps`` of a
        decode is something else: the frame at which the search first appended a label).  A row no path fits (more labels than frames,
        repeats that need blanks there is no room for, labels the rows rule out) has score ``-inf`` and zero spans.

        ``beam_results`` [B, R, L] / ``out_lens`` [B, R]: any label tensor and its lengths -- what ``decode``, ``decode_device`` and
        ``decode_padded`` return, with or without ``n_best``.  CPU or device tensors; the results are on the device when ``beam_results``
        is, otherwise CPU.  Follows the decoder's ``blank_id`` and input mode; half dtypes on the device are read as they are.
        ``blank_skip`` plays no part: the labels of a filtered decode are aligned on the original frames.  Raises ``ValueError`` for a row
        with a label outside the vocabulary, a blank label or a length outside [0, L]."""
        on_device = beam_results.is_cuda
        starts, ends, scores = self._score_rows("align", _native.lib.ctcd_ctc_align, probs, seq_lens, beam_results, out_lens,
                                                ((True, torch.int32), (True, torch.int32), (False, torch.float32)))
        if on_device or scores.numel() == 0:
            return (starts, ends, scores) if on_device else (starts.cpu(), ends.cpu(), scores.cpu())
        return _to_host((starts, ends, scores))

    def set_align_scratch(self, nbytes=0):
        """The budget of ``align``'s back-pointer scratch in bytes (include/ctcdecode_amd.h ctcd_set_align_scratch); 0 = the default.
        The persistent workgroups of a call are as many as the budget has slots for, at least one; the results do not depend on it."""
        _native.check(_native.lib.ctcd_set_align_scratch(self._handle, int(nbytes)))

    def last_align_grid(self):
        """Test hook: the workgroups the last ``align`` launched."""
        return int(_native.lib.ctcd_last_align_grid(self._handle))

    def log_likelihood(self, probs, seq_lens, beam_results, out_lens):
        """The CTC log-likelihood on the device (include/ctcdecode_amd.h "CTC log-likelihood"): for every row
        ``beam_results[b, r, :out_lens[b, r]]``, ``log P(y | x)`` -- the sum over ALL alignments of its labels through the rows
        ``probs[b, :seq_lens[b]]``, by the forward algorithm in float32, defined bit for bit.  Returns float32 [B, R]; ``-inf`` for a row
        no alignment fits.  Unlike ``beam_scores`` it does not depend on ``beam_width``, ``cutoff_top_n`` or ``blank_skip``.

        To re-rank an n-best list, sort each item's rows by this value (plus whatever a language model adds), greatest first: it is
        comparable across beam widths and decoders, and ``exp`` of it is the model's posterior of the whole transcript.
        ``log_likelihood - align(...)[2]`` is >= 0 and says how much of that mass lies outside the single best alignment (0: one
        alignment holds all of it).

        Tensor handling is that of ``align``: any label tensor and its lengths, CPU or device; the result is on the device when
        ``beam_results`` is, otherwise CPU.  Follows the decoder's ``blank_id`` and input mode; half dtypes on the device are read as they
        are.  Raises ``ValueError`` for a row with a label outside the vocabulary, a blank label or a length outside [0, L]."""
        on_device = beam_results.is_cuda
        loglik, = self._score_rows("log_likelihood", _native.lib.ctcd_ctc_loglik, probs, seq_lens, beam_results, out_lens, ((False, torch.float32),))
        return loglik if on_device else loglik.cpu()

    def set_loglik_grid(self, n=0):
        """The most workgroups a launch of ``log_likelihood`` uses (include/ctcdecode_amd.h ctcd_set_loglik_grid); 0 = the default, the
        workgroups the device holds at once.  The results do not depend on it."""
        _native.check(_native.lib.ctcd_set_loglik_grid(self._handle, int(n)))

    def last_loglik_grid(self):
        """Test hook: the workgroups of the widest launch of the last ``log_likelihood``."""
        return int(_native.lib.ctcd_last_loglik_grid(self._handle))

    def label_posteriors(self, probs, seq_lens, beam_results, out_lens):
        """CTC forward-backward per label on the device (include/ctcdecode_amd.h "Label posteriors"): for every label ``i`` of every row
        ``beam_results[b, r, :out_lens[b, r]]``, what the model's posterior over ALL alignments of the row through ``probs[b, :seq_lens[b]]``
        says about it.  Returns ``(peaks, occupancy, confidence, loglik)``:

        * ``peaks`` int32 [B, R, L]: the frame at which the label's posterior is greatest (the first such frame);
        * ``occupancy`` float32 [B, R, L]: the expected number of frames the label occupies;
        * ``confidence`` float32 [B, R, L]: the posterior-weighted mean of the model's probability of the label over the frames it
          occupies, in [0, 1] -- the soft form of averaging frame confidences over a hard alignment, low when the label is carried by
          frames that do not vote for it;
        * ``loglik`` float32 [B, R]: the row's log-likelihood, bit for bit what ``log_likelihood`` returns.

        The per-label outputs are 0 at or beyond a row's length, and for a row no alignment fits (``loglik`` = ``-inf``).  All four are
        defined bit for bit in float32.  Tensor handling is that of ``align`` and ``log_likelihood``: any label tensor and its lengths,
        CPU or device; the results are on the device when ``beam_results`` is, otherwise CPU.  Follows the decoder's ``blank_id`` and
        input mode; half dtypes on the device are read as they are.  Raises ``ValueError`` for a row with a label outside the
        vocabulary, a blank label or a length outside [0, L]."""
        on_device = beam_results.is_cuda
        outs = self._score_rows("label_posteriors", _native.lib.ctcd_ctc_posteriors, probs, seq_lens, beam_results, out_lens,
                                ((True, torch.int32), (True, torch.float32), (True, torch.float32), (False, torch.float32)))
        return tuple(outs) if on_device else tuple(o.cpu() for o in outs)

    def set_posterior_scratch(self, nbytes=0):
        """The budget of ``label_posteriors``' scratch in bytes (include/ctcdecode_amd.h ctcd_set_posterior_scratch); 0 = the default.
        The persistent workgroups of a call are as many as the budget has slots for, at least one; the results do not depend on it."""
        _native.check(_native.lib.ctcd_set_posterior_scratch(self._handle, int(nbytes)))

    def last_posterior_grid(self):
        """Test hook: the workgroups the last ``label_posteriors`` launched."""
        return int(_native.lib.ctcd_last_posterior_grid(self._handle))

    def greedy_decode_device(self, probs, seq_lens=None, details=False):
        """Greedy (best-path) CTC decoding on the device (include/ctcdecode_amd.h "Greedy decode"): every frame's most probable label,
        repeats collapsed, blanks dropped, in one read of ``probs``.  Returns ``(beam_results [B, 1, T] int32, scores [B, 1] float32,
        timesteps [B, 1, T] int32, out_lens [B, 1] int32)`` in HBM on the decoder's device, asynchronous on the current stream -- the
        order and dtypes of ``decode_device``, so the result goes straight into ``align``, ``log_likelihood`` and ``label_posteriors``.
        ``timesteps[b, 0, i]`` is the frame that emits label ``i``; positions at or beyond ``out_lens`` are 0.  ``scores`` is the path's
        log-probability, the float32 sum of the winners' values in frame order: the sign and the bits of ``align``'s score for that row,
        not the sign convention of ``decode``'s ``beam_scores``.  With ``details=True`` two more tensors follow: ``ends`` int32
        [B, 1, T], the last frame of each label's run, and ``label_scores`` float32 [B, 1, T], the greatest log-probability over it.

        Follows the decoder's ``blank_id`` and input mode (raw logits are normalised per frame without a copy of the input); half
        dtypes on the device are read as they are.  No language model, no ``cutoff_top_n`` / ``cutoff_prob`` and no ``blank_skip`` take
        part."""
        if probs.dim() != 3:
            raise ValueError("probs must be [batch, time, labels]")
        probs = _input_rows(self, probs)
        B, T, V = probs.shape
        if V != self._num_labels:
            raise ValueError("probs.shape[2] (%d) does not match the number of labels (%d)" % (V, self._num_labels))
        if not 0 <= int(self._blank_id) < V:
            raise ValueError("ctcdecode_amd: blank_id must index the vocabulary")
        if seq_lens is not None:
            seq_lens = seq_lens.to(device=self._device, dtype=torch.int32).contiguous()
            if seq_lens.numel() != B:
                raise ValueError("seq_lens must have one entry per batch item")
        with torch.cuda.device(self._device):
            tokens = torch.empty((B, 1, T), dtype=torch.int32, device=self._device)
            starts = torch.empty((B, 1, T), dtype=torch.int32, device=self._device)
            ends = torch.empty((B, 1, T), dtype=torch.int32, device=self._device) if details else None
            label_scores = torch.empty((B, 1, T), dtype=torch.float32, device=self._device) if details else None
            scores = torch.empty((B, 1), dtype=torch.float32, device=self._device)
            out_lens = torch.empty((B, 1), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(_native.lib.ctcd_greedy_decode(
                self._handle, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, B, T, V, int(self._blank_id), self._log_probs,
                tokens.data_ptr(), starts.data_ptr(), ends.data_ptr() if details else None, label_scores.data_ptr() if details else None,
                scores.data_ptr(), out_lens.data_ptr(), stream))
        return (tokens, scores, starts, out_lens, ends, label_scores) if details else (tokens, scores, starts, out_lens)

    def greedy_decode(self, probs, seq_lens=None):
        """``greedy_decode_device`` with the four tensors on the CPU: ``(beam_results [B, 1, T], scores [B, 1], timesteps [B, 1, T],
        out_lens [B, 1])``, the order and dtypes of ``decode``."""
        outs = self.greedy_decode_device(probs, seq_lens)
        return tuple(o.cpu() for o in outs) if outs[0].numel() == 0 else tuple(_to_host(outs))

    def edit_distance(self, beam_results, out_lens, references=None, ref_lens=None):
        """Levenshtein distances on the device (include/ctcdecode_amd.h "Edit distance"): ``D[b, i, j]``, int32 [B, R, Q], is the least
        number of insertions, deletions and substitutions that turn ``beam_results[b, i, :out_lens[b, i]]`` into
        ``references[b, j, :ref_lens[b, j]]``.  Tokens are compared as int32 values and nothing else: no vocabulary and no ``blank_id``
        take part, so word ids give word-level distances.  The arithmetic is integer and the result exact.

        ``references`` [B, Q, Lq] with ``ref_lens`` [B, Q], or [B, Lq] with ``ref_lens`` [B], which is read as Q = 1.
        ``references=None`` selects pairwise mode: every row of an item against every other row of it, [B, R, R] -- symmetric, a zero
        diagonal, each pair computed once.  Tensors may be on the CPU or the device and of any integer dtype (they are cast to int32);
        the result is on the device when ``beam_results`` is, otherwise CPU, as with ``align``.

        ``D[:, :, 0].argmin(1)`` is the oracle row of an n-best list against one reference, so there is no method for it.  Error rates
        are ``D / ref_lens``.  Rows of a decode beyond its number of results are empty rows and count as such: their distance to a
        reference is the reference's length.

        The shorter row of a pair is held in one wave's registers: ``min(L, Lq) > 2048`` raises ``NotImplementedError`` (the longer
        side is not bounded).  A length outside [0, L] (references: [0, Lq]) raises ``ValueError``."""
        if beam_results.dim() != 3 or out_lens.dim() != 2 or tuple(out_lens.shape) != tuple(beam_results.shape[:2]):
            raise ValueError("beam_results must be [batch, rows, labels] and out_lens [batch, rows]")
        on_device = beam_results.is_cuda
        B, R, L = (int(v) for v in beam_results.shape)
        pairwise = references is None
        if pairwise:
            if ref_lens is not None:
                raise ValueError("ref_lens given without references")
            Q, Lq = R, L
        else:
            if ref_lens is None:
                raise ValueError("references need ref_lens")
            if references.dim() == 2:
                references, ref_lens = references.unsqueeze(1), ref_lens.reshape(-1, 1)
            if references.dim() != 3 or ref_lens.dim() != 2 or tuple(ref_lens.shape) != tuple(references.shape[:2]):
                raise ValueError("references must be [batch, refs, labels] or [batch, labels], and ref_lens [batch, refs] or [batch]")
            if references.shape[0] != B:
                raise ValueError("references.shape[0] (%d) does not match the batch (%d)" % (references.shape[0], B))
            Q, Lq = int(references.shape[1]), int(references.shape[2])
        x = beam_results.to(device=self._device, dtype=torch.int32).contiguous()
        x_lens = out_lens.to(device=self._device, dtype=torch.int32).contiguous()
        with torch.cuda.device(self._device):
            y = y_lens = None
            if not pairwise:
                y = references.to(device=self._device, dtype=torch.int32).contiguous()
                y_lens = ref_lens.to(device=self._device, dtype=torch.int32).contiguous()
                if y.numel() == 0:  # (an empty tensor has no address, and a NULL y would select pairwise mode: a word that is never read)
                    y = torch.zeros((1,), dtype=torch.int32, device=self._device)
            out = torch.empty((B, R, Q), dtype=torch.int32, device=self._device)
            status = torch.zeros((max(B, 1),), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(_native.lib.ctcd_edit_distance(self._handle, x.data_ptr(), x_lens.data_ptr(), B, R, L, None if pairwise else y.data_ptr(),
                                                         None if pairwise else y_lens.data_ptr(), Q, Lq, out.data_ptr(), status.data_ptr(), stream))
            bad = torch.nonzero(status[:B]).flatten().tolist() if B else []
        if bad:
            raise ValueError("ctcdecode_amd: edit_distance: items %s have a row with a length outside [0, %d]%s (CTCD_ALIGN_BAD_ROW)"
                             % (bad[:8], L, "" if pairwise else " (references: [0, %d])" % Lq))
        return out if on_device else out.cpu()

    def last_edit_pairs(self):
        """Test hook: the distances the last ``edit_distance`` computed -- B x R x Q, or B x R x (R - 1) / 2 in pairwise mode."""
        return int(_native.lib.ctcd_last_edit_pairs(self._handle))

    def set_edit_grid(self, n=0):
        """The most workgroups the launch of ``edit_distance`` uses (include/ctcdecode_amd.h ctcd_set_edit_grid); 0 = the default, two
        per compute unit.  The results do not depend on it."""
        _native.check(_native.lib.ctcd_set_edit_grid(self._handle, int(n)))

    def last_edit_grid(self):
        """Test hook: the workgroups the last ``edit_distance`` launched."""
        return int(_native.lib.ctcd_last_edit_grid(self._handle))

    def _edit_rows(self, beam_results, out_lens, references, ref_lens):
        """The tensor handling ``edit_counts`` and ``edit_align`` share (that of ``edit_distance``).  -> (x, x_lens, y, y_lens, B, R, L,
        Q, Lq) on the decoder's device, int32 and contiguous; y and y_lens are None in pairwise mode."""
        if beam_results.dim() != 3 or out_lens.dim() != 2 or tuple(out_lens.shape) != tuple(beam_results.shape[:2]):
            raise ValueError("beam_results must be [batch, rows, labels] and out_lens [batch, rows]")
        B, R, L = (int(v) for v in beam_results.shape)
        x = beam_results.to(device=self._device, dtype=torch.int32).contiguous()
        x_lens = out_lens.to(device=self._device, dtype=torch.int32).contiguous()
        if references is None:
            if ref_lens is not None:
                raise ValueError("ref_lens given without references")
            return x, x_lens, None, None, B, R, L, R, L
        if ref_lens is None:
            raise ValueError("references need ref_lens")
        if references.dim() == 2:
            references, ref_lens = references.unsqueeze(1), ref_lens.reshape(-1, 1)
        if references.dim() != 3 or ref_lens.dim() != 2 or tuple(ref_lens.shape) != tuple(references.shape[:2]):
            raise ValueError("references must be [batch, refs, labels] or [batch, labels], and ref_lens [batch, refs] or [batch]")
        if references.shape[0] != B:
            raise ValueError("references.shape[0] (%d) does not match the batch (%d)" % (references.shape[0], B))
        Q, Lq = int(references.shape[1]), int(references.shape[2])
        y = references.to(device=self._device, dtype=torch.int32).contiguous()
        y_lens = ref_lens.to(device=self._device, dtype=torch.int32).contiguous()
        if y.numel() == 0:  # (an empty tensor has no address, and a NULL y selects pairwise mode: a word that is never read)
            y = torch.zeros((1,), dtype=torch.int32, device=self._device)
        return x, x_lens, y, y_lens, B, R, L, Q, Lq

    def _edit_raise(self, what, status, B, L, Lq, pairwise):
        bad = torch.nonzero(status[:B]).flatten().tolist() if B else []
        if bad:
            raise ValueError("ctcdecode_amd: %s: items %s have a row with a length outside [0, %d]%s (CTCD_ALIGN_BAD_ROW)"
                             % (what, bad[:8], L, "" if pairwise else " (references: [0, %d])" % Lq))

    def edit_counts(self, beam_results, out_lens, references=None, ref_lens=None):
        """How an edit distance splits (include/ctcdecode_amd.h "Edit operations"): int32 [B, R, Q, 4] = ``(hits, substitutions,
        deletions, insertions)`` of turning the reference ``references[b, j]`` into the hypothesis ``beam_results[b, i]`` -- an
        insertion is a hypothesis token without a partner, a deletion a reference token without one.  Among the alignments of least
        distance the counts are those with the fewest substitutions (the most hits); ``S + Del + I`` is ``edit_distance``,
        ``H + S + I`` the hypothesis' length and ``H + S + Del`` the reference's.

        Arguments, modes and tensor handling are ``edit_distance``'s.  Pairwise mode (``references=None``) gives [B, R, R, 4]:
        ``[b, i, j]`` takes row ``i`` as the hypothesis, ``[b, j, i]`` has deletions and insertions exchanged, the diagonal is
        ``(len, 0, 0, 0)``.  ``min(L, Lq) > 2048`` or ``max(L, Lq) > 262144`` raises ``NotImplementedError``; a length outside its
        bounds raises ``ValueError``."""
        on_device = beam_results.is_cuda
        x, x_lens, y, y_lens, B, R, L, Q, Lq = self._edit_rows(beam_results, out_lens, references, ref_lens)
        pairwise = y is None
        with torch.cuda.device(self._device):
            out = torch.empty((B, R, Q, 4), dtype=torch.int32, device=self._device)
            status = torch.zeros((max(B, 1),), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(_native.lib.ctcd_edit_counts(self._handle, x.data_ptr(), x_lens.data_ptr(), B, R, L, None if pairwise else y.data_ptr(),
                                                       None if pairwise else y_lens.data_ptr(), Q, Lq, out.data_ptr(), status.data_ptr(), stream))
            self._edit_raise("edit_counts", status, B, L, Lq, pairwise)
        return out if on_device else out.cpu()

    def edit_align(self, beam_results, out_lens, references, ref_lens):
        """The token alignment behind an edit distance (include/ctcdecode_amd.h "Edit operations").  Returns ``(hyp_to_ref int32
        [B, R, Q, L], ref_to_hyp int32 [B, R, Q, Lq], counts int32 [B, R, Q, 4])``: ``hyp_to_ref[b, i, j, p]`` is the position in
        ``references[b, j]`` that token ``p`` of ``beam_results[b, i]`` stands against -- a hit or a substitution -- or -1 if the
        token is an insertion or ``p`` is at or beyond the row's length; ``ref_to_hyp`` is the same from the reference's side (-1: a
        deletion); ``counts`` is what ``edit_counts`` returns.  Of the alignments of least distance it is one with the fewest
        substitutions, and among those the canonical one of the header: walking back from the ends, a pair is preferred to an
        insertion and an insertion to a deletion.  ``timesteps.gather(-1, ref_to_hyp.clamp_min(0))`` carries a hypothesis' time steps
        onto the reference.

        ``references`` are required (there is no pairwise mode); tensor handling and errors are ``edit_counts``'.  The walk's
        directions live in decoder-owned scratch (``set_edit_scratch``); a call whose single slot does not fit the budget raises
        ``NotImplementedError``."""
        if references is None:
            raise ValueError("edit_align needs references: alignments are not provided in pairwise mode")
        on_device = beam_results.is_cuda
        x, x_lens, y, y_lens, B, R, L, Q, Lq = self._edit_rows(beam_results, out_lens, references, ref_lens)
        with torch.cuda.device(self._device):
            h2r = torch.empty((B, R, Q, L), dtype=torch.int32, device=self._device)
            r2h = torch.empty((B, R, Q, Lq), dtype=torch.int32, device=self._device)
            counts = torch.empty((B, R, Q, 4), dtype=torch.int32, device=self._device)
            status = torch.zeros((max(B, 1),), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(_native.lib.ctcd_edit_align(self._handle, x.data_ptr(), x_lens.data_ptr(), B, R, L, y.data_ptr(), y_lens.data_ptr(), Q, Lq,
                                                      h2r.data_ptr() if h2r.numel() else None, r2h.data_ptr() if r2h.numel() else None, counts.data_ptr(),
                                                      status.data_ptr(), stream))
            self._edit_raise("edit_align", status, B, L, Lq, False)
        outs = (h2r, r2h, counts)
        return outs if on_device else tuple(o.cpu() for o in outs)

    def set_edit_scratch(self, nbytes=0):
        """The budget of ``edit_align``'s back-pointer scratch in bytes (include/ctcdecode_amd.h ctcd_set_edit_scratch); 0 = the
        default, 1 GiB.  A call runs as many waves as the budget has slots for; the results do not depend on it."""
        _native.check(_native.lib.ctcd_set_edit_scratch(self._handle, int(nbytes)))

    def last_edit_slots(self):
        """Test hook: the back-pointer slots (waves with work) of the last ``edit_align``."""
        return int(_native.lib.ctcd_last_edit_slots(self._handle))

    def mbr_select(self, beam_results, out_lens, log_weights):
        """Minimum-Bayes-risk selection from an n-best list: for every item the row with the least expected edit distance to the other
        rows.  Returns ``(index int64 [B], risk float64 [B, R])``, on the device when ``beam_results`` is, otherwise CPU.

        ``D`` = pairwise ``edit_distance``; ``w = softmax(log_weights[b])`` in float64; ``risk[b, i] = sum_j w[b, j] * D[b, i, j]``;
        ``index[b]`` is the smallest ``i`` of least risk.  Rows with ``log_weights == -inf`` weigh nothing, get risk ``+inf`` and are
        never chosen; an item without a finite weight gets index ``-1`` and all risks ``+inf``.  The distances come from
        ``edit_distance``, which reads its status words on the host (and so waits for the device, and raises ``ValueError`` for a bad
        length); everything after them is plain torch on the device, with no further host read.

        The natural weights are ``log_likelihood(probs, seq_lens, beam_results, out_lens)`` (plus whatever a language model adds).
        Pass ``-inf`` for rows beyond a decode's result count: such rows are empty, and an empty row must not vote."""
        if log_weights.dim() != 2 or tuple(log_weights.shape) != tuple(beam_results.shape[:2]):
            raise ValueError("log_weights must be [batch, rows], one weight per row of beam_results")
        on_device = beam_results.is_cuda
        D = self.edit_distance(beam_results.to(self._device), out_lens).to(torch.float64)
        lw = log_weights.to(device=self._device, dtype=torch.float64)
        live = lw > float("-inf")
        any_live = live.any(dim=1)
        top = torch.where(live, lw, torch.full_like(lw, -1.0e308)).max(dim=1, keepdim=True).values if lw.shape[1] else lw[:, :0]
        e = torch.where(live, torch.exp(torch.where(live, lw - top, torch.zeros_like(lw))), torch.zeros_like(lw))
        w = e / e.sum(dim=1, keepdim=True).clamp_min(1.0e-300)
        inf = torch.full_like(lw, float("inf"))
        risk = torch.where(live, (D * w.unsqueeze(1)).sum(dim=2), inf)
        if lw.shape[1]:
            rows = torch.arange(lw.shape[1], dtype=torch.int64, device=self._device).expand_as(risk)
            first = torch.where(risk == risk.min(dim=1, keepdim=True).values, rows, torch.full_like(rows, lw.shape[1])).min(dim=1).values
            index = torch.where(any_live, first, torch.full_like(first, -1))
        else:
            index = torch.full((lw.shape[0],), -1, dtype=torch.int64, device=self._device)
        return (index, risk) if on_device else (index.cpu(), risk.cpu())

    def decode_padded(self, probs, seq_lens=None, n_best=None):
        """The same call with the padded [B, K, T] tensors crossing PCIe (the delivery of round 1; kept for comparison); with ``n_best``
        the [B, n, T] ones."""
        return _to_host(self.decode_device(probs, seq_lens, n_best=n_best))

    def decode_compact(self, probs, seq_lens=None):
        """Device-resident compact results: (c_hdr [B,4], c_ent [B,K,4], c_labels [n], scores [B,K], out_lens [B,K]) in HBM --
        what a rank ships to the gathering rank; ``expand_compact`` rebuilds the padded tensors there."""
        if probs.dim() != 3:
            raise ValueError("probs must be [batch, time, labels]")
        probs = _input_rows(self, probs)
        B, T, V = probs.shape
        if V != self._num_labels:
            raise ValueError("probs.shape[2] (%d) does not match the number of labels (%d)" % (V, self._num_labels))
        if seq_lens is not None:
            seq_lens = seq_lens.to(device=self._device, dtype=torch.int32).contiguous()
        K = self._beam_width
        cap = int(_native.lib.ctcd_compact_label_capacity(B, K, T))
        log_mode, kept = self._log_probs, None
        sk = self._skip_rows(probs, seq_lens)
        if sk is not None:  # blank_skip: the decode sees the kept rows and their counts
            probs, seq_lens, kept, log_mode = sk
        with torch.cuda.device(self._device):
            if getattr(self, "_c_labels", None) is None or self._c_labels.numel() < max(cap, 1):
                self._c_labels = torch.empty((max(cap, 1),), dtype=torch.int32, device=self._device)  # worst case, reused
            hdr = torch.empty((B, 4), dtype=torch.int32, device=self._device)
            ent = torch.empty((B, K, 4), dtype=torch.int32, device=self._device)
            cnt = torch.empty((1,), dtype=torch.int32, device=self._device)
            scores = torch.empty((B, K), dtype=torch.float32, device=self._device)
            out_len = torch.empty((B, K), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            self._check(_native.lib.ctcd_beam_decode_compact(
                self._handle, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, B, T, V, K, self._num_processes,
                float(self._cutoff_prob), int(self.cutoff_top_n), int(self._blank_id), log_mode,
                self._scorer.handle if self._scorer is not None else None, hdr.data_ptr(), ent.data_ptr(), self._c_labels.data_ptr(),
                cnt.data_ptr(), cap, scores.data_ptr(), out_len.data_ptr(), None, stream))
            self._last_batch = B  # (last_launch_order: the batch of the last call that was queued)
            if kept is not None and K > 0:  # the records' frame numbers back to original frames, behind the decode on its stream
                _native.check(_native.lib.ctcd_remap_compact(self._handle, hdr.data_ptr(), ent.data_ptr(), self._c_labels.data_ptr(), kept.data_ptr(),
                                                             seq_lens.data_ptr(), B, K, T, stream))
            _native.check(_native.lib.ctcd_check_status(self._handle, B))
            n = int(cnt.item())
        # (an owned copy: the per-decoder buffer is overwritten by this decoder's next call, possibly while an asynchronous
        #  gather of this batch still reads the labels)
        return hdr, ent, self._c_labels[:n].clone(), scores, out_len

    def decode_compact_async(self, probs, seq_lens=None):
        """``decode_compact`` without waiting: the kernel, then the copies of the status words and of the label count into
        page-locked memory, are enqueued on the current stream and an event is recorded behind them.  Returns a ticket for
        ``finish_compact``; the caller may queue the NEXT batch (on another decoder object: this one's workspace is in use)
        before looking at this one -- how a serving loop keeps the GPU busy while the host handles the previous results.
        With a callback scorer the call BLOCKS until the decode is done: the callback is served on the calling thread."""
        if probs.dim() != 3:
            raise ValueError("probs must be [batch, time, labels]")
        probs = _input_rows(self, probs)
        B, T, V = probs.shape
        if V != self._num_labels:
            raise ValueError("probs.shape[2] (%d) does not match the number of labels (%d)" % (V, self._num_labels))
        if seq_lens is not None:
            seq_lens = seq_lens.to(device=self._device, dtype=torch.int32).contiguous()
        K = self._beam_width
        cap = int(_native.lib.ctcd_compact_label_capacity(B, K, T))
        log_mode, kept = self._log_probs, None
        sk = self._skip_rows(probs, seq_lens)
        if sk is not None:  # blank_skip: the decode sees the kept rows and their counts
            probs, seq_lens, kept, log_mode = sk
        with torch.cuda.device(self._device):
            if getattr(self, "_c_labels", None) is None or self._c_labels.numel() < max(cap, 1):
                self._c_labels = torch.empty((max(cap, 1),), dtype=torch.int32, device=self._device)  # worst case, reused
            hdr = torch.empty((B, 4), dtype=torch.int32, device=self._device)
            ent = torch.empty((B, K, 4), dtype=torch.int32, device=self._device)
            cnt = torch.empty((1,), dtype=torch.int32, device=self._device)
            scores = torch.empty((B, K), dtype=torch.float32, device=self._device)
            out_len = torch.empty((B, K), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device)
            self._check(_native.lib.ctcd_beam_decode_compact(
                self._handle, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, B, T, V, K, self._num_processes,
                float(self._cutoff_prob), int(self.cutoff_top_n), int(self._blank_id), log_mode,
                self._scorer.handle if self._scorer is not None else None, hdr.data_ptr(), ent.data_ptr(), self._c_labels.data_ptr(),
                cnt.data_ptr(), cap, scores.data_ptr(), out_len.data_ptr(), None, stream.cuda_stream))
            self._last_batch = B  # (last_launch_order: the batch of the last call that was queued)
            if kept is not None and K > 0:  # the records' frame numbers back to original frames, behind the decode on its stream
                _native.check(_native.lib.ctcd_remap_compact(self._handle, hdr.data_ptr(), ent.data_ptr(), self._c_labels.data_ptr(), kept.data_ptr(),
                                                             seq_lens.data_ptr(), B, K, T, stream.cuda_stream))
            status = torch.empty((max(B, 1),), dtype=torch.int32, pin_memory=True)
            cnt_host = torch.empty((1,), dtype=torch.int32, pin_memory=True)
            _native.check(_native.lib.ctcd_fetch_status_async(self._handle, B, status.data_ptr(), stream.cuda_stream))
            cnt_host.copy_(cnt, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        return dict(B=B, hdr=hdr, ent=ent, labels=self._c_labels, cnt=cnt, scores=scores, lens=out_len, status=status, cnt_host=cnt_host,
                    event=ev, keep=(probs, seq_lens, kept))

    def finish_compact(self, ticket):
        """Waits for a ``decode_compact_async`` batch (its own event only, not the stream) and returns what ``decode_compact``
        returns: (c_hdr, c_ent, c_labels[:n], scores, out_lens)."""
        ticket["event"].synchronize()
        st = ticket["status"][:ticket["B"]]
        if ticket["B"] and bool((st != 0).any()):
            b = int((st != 0).nonzero()[0])
            raise _native.NativeError("ctcdecode_amd: decoder status %d for item %d" % (int(st[b]), b))
        n = int(ticket["cnt_host"][0])
        with torch.cuda.device(self._device):
            labels = ticket["labels"][:n].clone()  # owned: the decoder's label buffer belongs to its next call
        return ticket["hdr"], ticket["ent"], labels, ticket["scores"], ticket["lens"]

    def expand_compact(self, hdr, ent, labels, T, n_best=None):
        """(c_hdr, c_ent, c_labels) of any number of items -> (output [B,K,T], timesteps [B,K,T]) in HBM.  ``n_best`` = n: rows 0 .. n-1
        alone, [B,n,T], zero outside the valid region; every record index is checked on the device, a malformed record zeroes the rows
        that depend on it and raises NativeError here (this form waits for the expansion)."""
        B, K = int(ent.shape[0]), int(ent.shape[1])
        n_best = _n_best(n_best, K)
        if n_best is not None:
            with torch.cuda.device(self._device):
                output = torch.empty((B, n_best, T), dtype=torch.int32, device=self._device)
                timesteps = torch.empty((B, n_best, T), dtype=torch.int32, device=self._device)
                status = torch.zeros((max(B, 1),), dtype=torch.int32, device=self._device)
                n_labels = int(labels.numel())
                labels = labels.contiguous() if n_labels else torch.zeros((1,), dtype=torch.int32, device=self._device)  # (no label at all: a non-null pointer)
                stream = torch.cuda.current_stream(self._device).cuda_stream
                _native.check(_native.lib.ctcd_expand_compact_nbest(self._handle, hdr.contiguous().data_ptr(), ent.contiguous().data_ptr(), labels.data_ptr(),
                                                                    n_labels, B, K, T, n_best, output.data_ptr(), timesteps.data_ptr(),
                                                                    status.data_ptr(), stream))
                st = status.cpu()
            if bool((st != 0).any()):
                b = int((st != 0).nonzero()[0])
                raise _native.NativeError("ctcdecode_amd: malformed compact record (status %d) for item %d" % (int(st[b]), b))
            return output, timesteps
        with torch.cuda.device(self._device):
            output = torch.empty((B, K, T), dtype=torch.int32, device=self._device)
            timesteps = torch.empty((B, K, T), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(_native.lib.ctcd_expand_compact(self._handle, hdr.contiguous().data_ptr(), ent.contiguous().data_ptr(),
                                                          labels.contiguous().data_ptr(), B, K, T, output.data_ptr(), timesteps.data_ptr(), stream))
        return output, timesteps

    def character_based(self):  # ctcdecode/__init__.py:125-136: None without a scorer
        return bool(_native.lib.ctcd_scorer_is_character_based(self._scorer.handle)) if self._scorer else None

    def max_order(self):
        return int(_native.lib.ctcd_scorer_max_order(self._scorer.handle)) if self._scorer else None

    def dict_size(self):
        return int(_native.lib.ctcd_scorer_dict_size(self._scorer.handle)) if self._scorer else None

    def reset_params(self, alpha, beta):
        if self._scorer is not None:
            _native.check(_native.lib.ctcd_scorer_reset_params(self._scorer.handle, float(alpha), float(beta)))

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                _native.destroy(_native.lib.ctcd_destroy, h)
            except Exception:
                pass
            self._handle = None


class DecodePipeline(object):
    """A serving loop's launches kept ``inflight`` at a time, each on a HIP stream and a decoder of its own (round 5).

    One utterance occupies one workgroup -- one CU in the kernel's default build -- and the time axis of an utterance cannot
    be split, so (a) a batch with fewer utterances than the GPU has CUs leaves the other CUs idle for the whole launch, and
    (b) any launch lasts as long as its slowest utterance (the ones with the most exact ``std::nth_element`` replays: 10-15 %
    above the mean on random rows) while the CUs of the finished ones idle.  With two launches in flight the next batch's
    workgroups take those CUs: the rule is ``inflight_for(batch)`` = 2 below the CU count (``min_shard`` is the same rule
    for ranks: ctcdecode_amd/distributed.py), and 2 is also what hides the stragglers of full batches.  No CU is shared:
    this is the default build of the kernel (``cu_sharing=True`` asks for the two-workgroups-per-CU build instead, which
    pays off from three full batches in flight: bench.py ``pipelined``).

        pipe = DecodePipeline(lambda: CTCBeamDecoder(labels, beam_width=100, log_probs_input=True), inflight=2)
        tickets = [pipe.submit(batch) for batch in batches]      # asynchronous; at most `inflight` are in flight
        results = [pipe.result(t) for t in tickets]              # (output, scores, timesteps, out_lens) in HBM, in order

    ``submit`` waits for the slot's previous launch if its status has not been looked at yet; tickets stay fetchable in any
    order.  A batch that failed (a status word, a scorer callback's exception) raises from ``result`` of ITS ticket -- every time it
    is asked -- and from ``drain``; it never blocks its slot: the next ``submit`` there goes ahead.
    """

    def __init__(self, make_decoder, inflight=2, cu_sharing=False):
        if inflight < 1:
            raise ValueError("inflight must be at least 1")
        self._decs = [make_decoder() for _ in range(inflight)]
        self._device = self._decs[0]._device
        for d in self._decs:
            if d._device != self._device:
                raise ValueError("DecodePipeline: every decoder must sit on the same device")
            if cu_sharing:
                d.set_cu_sharing(1)
        self._streams = [torch.cuda.Stream(device=self._device) for _ in range(inflight)]
        self._pending = [None] * inflight  # per slot: the ticket whose status has not been looked at
        self._serial = 0

    @staticmethod
    def inflight_for(batch, device=None):
        """2 when a batch leaves CUs idle (fewer utterances than CUs), else 1 -- the partition rule of DESIGN.md section 7."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        return 2 if batch < torch.cuda.get_device_properties(dev).multi_processor_count else 1

    def submit(self, probs, seq_lens=None, n_best=None):
        """Queues a batch; ``n_best`` as in ``CTCBeamDecoder.decode_device``."""
        slot = self._serial % len(self._decs)
        n_best = _n_best(n_best, self._decs[slot]._beam_width)  # (refused before the slot's previous launch is waited for)
        if self._pending[slot] is not None:
            self._finish(self._pending[slot])
        dec, stream = self._decs[slot], self._streams[slot]
        stream.wait_stream(torch.cuda.current_stream(self._device))  # (the caller's tensors are ready on its own stream)
        with torch.cuda.stream(stream):
            res = dec.decode_device(probs, seq_lens, check=False, n_best=n_best)
            ev = torch.cuda.Event()
            ev.record(stream)
        # (the launch reads the caller's tensors on the side stream: they stay referenced until it has finished -- a tensor
        #  dropped by the caller right after submit() would otherwise go back to the caching allocator and be handed out again)
        ticket = {"slot": slot, "serial": self._serial, "res": res, "event": ev, "batch": int(probs.shape[0]), "done": False,
                  "inputs": (probs, seq_lens), "error": None}
        self._pending[slot] = ticket
        self._serial += 1
        return ticket

    def _finish(self, ticket):
        """Waits for the ticket's launch and looks at its status words once; a failure is kept on the ticket (raising from
        here left the slot pending for ever)."""
        if ticket["done"]:
            return
        slot = ticket["slot"]
        try:
            ticket["event"].synchronize()
            self._decs[slot]._check(_native.lib.ctcd_check_status(self._decs[slot]._handle, ticket["batch"]))
        except Exception as e:  # noqa: BLE001 (whatever decode_device would have raised)
            ticket["error"] = e
        finally:
            ticket["done"] = True
            ticket["inputs"] = None
            if self._pending[slot] is ticket:
                self._pending[slot] = None

    def result(self, ticket):
        """The four HBM tensors of a submitted batch (waits for its launch; raises what ``decode_device`` would have raised)."""
        self._finish(ticket)
        if ticket.get("error") is not None:
            raise ticket["error"]
        torch.cuda.current_stream(self._device).wait_event(ticket["event"])
        return ticket["res"]

    def drain(self):
        """Waits for everything in flight; raises the first failure among the batches nobody has asked about yet."""
        first = None
        for t in list(self._pending):
            if t is not None:
                self._finish(t)
                if first is None and t.get("error") is not None:
                    first = t["error"]
        if first is not None:
            raise first


class OnlineCTCBeamDecoder(object):
    """Streaming drop-in for ctcdecode/__init__.py:143-250 (no language model): feed an utterance chunk by chunk through a
    ``DecoderState``; results are produced for the items whose ``is_eos_s`` entry is True.  The beam and node pool of
    every stream stay in HBM between calls; ``timesteps`` count frames from the beginning of the stream.

    ``set_blank_skip(thr)`` (extension; off until it is called, and then the streaming path is exactly what it is without it; the
    constructor keeps the reference's parameters and does not take the setting): a threshold in (0, 1], as ``CTCBeamDecoder``'s
    ``blank_skip``: every chunk drops, on the device and before the beam search, the frames whose blank posterior is
    GREATER than the threshold.  A stream decodes the kept frames alone and reports every time step -- at its end, from ``peek`` and
    from ``commit`` -- as the kept frame's index among all frames it has been fed, so that, however the frames are cut into chunks,
    it returns what ``CTCBeamDecoder(blank_skip=thr)`` returns for the concatenation, bit for bit.  ``DecoderState.frames`` counts
    the frames decoded (the kept ones), ``DecoderState.frames_seen`` the frames fed.  The node pools are sized on the host from the
    chunk lengths, so a filtered ``decode`` call WAITS on the current stream for the kept counts of its chunk before it launches the
    decode: one small read per call; ``check=False`` still skips the wait for the status words behind it.  A stream adopts the filter
    at its first chunk; ``save`` of a filtered stream and ``restore`` on a filtering decoder raise ``NotImplementedError``
    (include/ctcdecode_amd.h "Blank-frame filter of live streams")."""

    def __init__(self, labels, model_path=None, alpha=0, beta=0, cutoff_top_n=40, cutoff_prob=1.0, beam_width=100,
                 num_processes=4, blank_id=0, log_probs_input=False, device=None, logits_input=False, scorer=None, compact_pool_above=None):
        self._blank_skip = None  # set_blank_skip
        self._filtered_once = False  # a chunk call has gone through the filter since (last_blank_skip)
        self._cutoff_top_n = cutoff_top_n
        self._beam_width = beam_width
        self._scorer = None
        self._num_processes = num_processes
        self._labels = list(labels)
        self._num_labels = len(labels)
        self._blank_id = blank_id
        # logits_input (extension, not in the reference): the input holds raw logits; the device normalises them with a
        # float32 log_softmax (include/ctcdecode_amd.h ctcd_log_softmax) before decoding
        self._log_probs = 2 if logits_input else (1 if log_probs_input else 0)
        self._cutoff_prob = cutoff_prob
        if not torch.cuda.is_available():
            raise RuntimeError("ctcdecode_amd: no HIP device visible; this decoder has no CPU path")
        self._device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())
        h = ctypes.c_void_p()
        _native.check(_native.lib.ctcd_create(ctypes.byref(h), self._device.index))
        self._handle = h
        # compact_pool_above (extension): a stream whose next chunk does not fit its node pool, and whose pool may hold at least this
        # many nodes, is compacted (see ``compact``) before it is allowed to double; None: streams only ever double
        if compact_pool_above is not None:
            if int(compact_pool_above) < 1:
                raise ValueError("compact_pool_above is a node count of at least 1 (None: off)")
            _native.check(_native.lib.ctcd_set_stream_compaction(self._handle, int(compact_pool_above)))
        if scorer is not None:
            self._scorer = _adopt_scorer(scorer, model_path, self._num_labels, self._device.index)
        elif model_path:  # ctcdecode/__init__.py:183-187
            self._scorer = _Scorer(alpha, beta, model_path, self._labels, self._device.index)

    def _check(self, rc):
        """``_native.check`` for the calls a scorer callback runs under: an exception raised inside the callback comes first."""
        if rc and self._scorer is not None and hasattr(self._scorer, "_raise_pending"):
            self._scorer._raise_pending()
        _native.check(rc)

    def set_threads(self, n):
        """Test hook (as CTCBeamDecoder.set_threads): threads per workgroup, 0 = the library's choice."""
        _native.check(_native.lib.ctcd_set_threads(self._handle, int(n)))

    def last_layout(self):
        """As CTCBeamDecoder.last_layout (the last chunk's launch)."""
        return int(_native.lib.ctcd_debug_last_layout(self._handle))

    def last_kernel(self):
        """As CTCBeamDecoder.last_kernel (the last chunk's launch)."""
        return _last_kernel(self._handle)

    def last_prepass(self):
        """As CTCBeamDecoder.last_prepass (the last chunk's pre-passes)."""
        return _last_prepass(self._handle)

    def set_scorer_wait(self, on=True):
        """As CTCBeamDecoder.set_scorer_wait."""
        _native.check(_native.lib.ctcd_set_scorer_wait(self._handle, 1 if on else 0))

    def set_scorer_filter(self, on=True):
        """As CTCBeamDecoder.set_scorer_filter."""
        _native.check(_native.lib.ctcd_set_scorer_filter(self._handle, 1 if on else 0))

    def last_scorer_pairs(self):
        """As CTCBeamDecoder.last_scorer_pairs."""
        return _last_scorer_pairs(self._handle)

    def set_blank_skip(self, thr):
        """The blank-frame filter of live streams (see the class): ``thr`` a threshold in (0, 1], checked as ``CTCBeamDecoder``'s
        ``blank_skip`` is, or None: off.  Call it before the decoder's streams are created and fed: a stream adopts the setting at its
        first chunk, and a stream that has frames under the other setting is refused (``ValueError``) and left unchanged.  The decoder
        does not know its live streams, so nothing stops a change while filtered streams are live: they are then refused by every call
        until the setting they adopted is back."""
        thr = _blank_skip_threshold(thr)
        if thr is None:
            _native.check(_native.lib.ctcd_set_stream_blank_skip(self._handle, 0, 0.0, 0.0))
        else:  # (the two float32 bounds of CTCBeamDecoder._skip_rows: probabilities | log-probabilities and logits)
            _native.check(_native.lib.ctcd_set_stream_blank_skip(self._handle, 1, _f32(thr), _f32(math.log(thr))))
        self._blank_skip = thr
        self._filtered_once = False

    def last_blank_skip(self):
        """As CTCBeamDecoder.last_blank_skip: (frames considered, frames kept) of the last chunk call's filter, or None if the filter
        is off or no call has filtered yet."""
        if self._blank_skip is None or not self._filtered_once:
            return None
        considered, kept = ctypes.c_longlong(0), ctypes.c_longlong(0)
        _native.check(_native.lib.ctcd_last_stream_blank_skip(self._handle, ctypes.byref(considered), ctypes.byref(kept)))
        return int(considered.value), int(kept.value)

    def decode(self, probs, states, is_eos_s, seq_lens=None, check=True):
        """Same contract as ctcdecode/__init__.py:189-238: returns CPU tensors (beam_results[B, R, L], beam_scores[B, K],
        timesteps[B, R, L], out_lens[B, K]) with R = most results of any item that ended (0 if none), L = longest beam.

        ``check=False`` (extension): a call in which no stream ends returns as soon as the chunk's kernel is queued on the
        current stream instead of waiting for its status words -- a serving loop feeds chunk after chunk without a host
        synchronisation in between; a failure surfaces at the next checked call (every call that ends a stream is one).
        After ``set_blank_skip`` every call -- ``check=False`` too -- waits on the current stream for the kept counts of its chunk before
        it launches the decode (the node pools are sized on the host); ``check=False`` then skips only the wait for the status words."""
        if probs.dim() != 3:
            raise ValueError("probs must be [batch, time, labels]")
        B, T, V = probs.shape
        if V != self._num_labels:
            raise ValueError("probs.shape[2] (%d) does not match the number of labels (%d)" % (V, self._num_labels))
        if len(states) != B or len(is_eos_s) != B:
            raise ValueError("states and is_eos_s need one entry per batch item")
        probs = _input_rows(self, probs)  # (bfloat16 / float16 chunks on the device: decoded as they are, as their float32 copies)
        lens_cpu = None
        if seq_lens is not None:
            lens_cpu = seq_lens.detach().cpu().to(torch.int32).contiguous()
        K = self._beam_width
        self._unchecked = 0  # (this call's launch takes over the status words)
        # (a serving loop calls this once per chunk with the same states: the per-call host work is kept small -- the array of
        #  state handles is rebuilt only when the list changes, nothing is allocated or read back unless a stream ends)
        # (the cache holds WEAK references: a strong list kept ended streams' HBM blocks alive until the next call with other
        #  states, and tied decoder and states into a cycle of objects with finalisers -- ADVICE r4)
        cache = getattr(self, "_ptr_cache", None)
        if cache is None or len(cache[0]) != B or any(r() is not st for r, st in zip(cache[0], states)):
            cache = ([weakref.ref(st) for st in states], (ctypes.c_void_p * max(B, 1))(*[st._ptr(self) for st in states]))
            self._ptr_cache = cache
        ptrs = cache[1]
        any_eos = any(is_eos_s)
        eos = (ctypes.c_ubyte * max(B, 1)).from_buffer_copy(bytes(bytearray(1 if e else 0 for e in is_eos_s)) or b"\0")
        out_T = 0
        if any_eos:
            for b in range(B):
                if is_eos_s[b]:
                    ln = T if lens_cpu is None else max(0, min(int(lens_cpu[b]), T))
                    out_T = max(out_T, int(_native.lib.ctcd_stream_frames(ptrs[b])) + ln)
        self._filtered_once = self._blank_skip is not None
        # (with blank_skip, compact records would have to hold indices among the frames SEEN in their 16 bits: the native bound)
        compact_ok = self._blank_skip is None or all(int(_native.lib.ctcd_stream_frames_seen(ptrs[b])) + T <= 65536 for b in range(B))
        if any_eos and not (self._scorer is not None and isinstance(self._scorer, CallbackScorer)) and out_T <= 65536 and V <= 65535 and compact_ok:
            # streams end: their results leave the GPU as compact records and are expanded on the host, straight into tensors of the
            # reference's sizes (binding.cpp:186-205) -- the allocator below is called once the kernel has run and R, L are known
            made = {}

            def alloc(_user, R, L, p_tok, p_ts):
                try:
                    pin = B * R * L > 0
                    made["tok"] = torch.empty((B, R, L), dtype=torch.int32, pin_memory=pin)
                    made["ts"] = torch.empty((B, R, L), dtype=torch.int32, pin_memory=pin)
                    p_tok[0] = made["tok"].data_ptr()
                    p_ts[0] = made["ts"].data_ptr()
                    return 0
                except Exception as e:  # (reported through the return code: no exception crosses the C frame)
                    made["error"] = e
                    return 1

            cb = _native.RESULT_ALLOC_FN(alloc)
            scores = torch.empty((B, K), dtype=torch.float32, pin_memory=True)
            out_len = torch.empty((B, K), dtype=torch.int32, pin_memory=True)
            nres = torch.empty((B,), dtype=torch.int32, pin_memory=True)
            R, L = ctypes.c_int(0), ctypes.c_int(0)
            with torch.cuda.device(self._device):
                stream = torch.cuda.current_stream(self._device).cuda_stream
                rc = _native.lib.ctcd_stream_decode_to_host(
                    self._handle, ptrs, eos, probs.data_ptr(), lens_cpu.data_ptr() if lens_cpu is not None else None, B, T, V, K, self._num_processes,
                    float(self._cutoff_prob), int(self._cutoff_top_n), int(self._blank_id), self._log_probs, cb, None,
                    scores.data_ptr(), out_len.data_ptr(), nres.data_ptr(), out_T, ctypes.byref(R), ctypes.byref(L), stream)
            self._ptr_cache = None  # (ended streams are not decoded again: the next call brings other states)
            if "error" in made:
                raise made["error"]
            self._check(rc)
            return made["tok"], scores, made["ts"], out_len
        with torch.cuda.device(self._device):
            scr = getattr(self, "_scratch", None)
            if scr is None or scr[0].shape[0] != B:
                scr = (torch.empty((B, K), dtype=torch.float32, device=self._device), torch.empty((B, K), dtype=torch.int32, device=self._device),
                       torch.empty((B,), dtype=torch.int32, device=self._device))
                self._scratch = scr
            scores, out_len, nres = scr
            output = torch.empty((B, K, out_T), dtype=torch.int32, device=self._device)
            timesteps = torch.empty((B, K, out_T), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            self._check(_native.lib.ctcd_stream_decode(
                self._handle, ptrs, eos, probs.data_ptr(), lens_cpu.data_ptr() if lens_cpu is not None else None, B, T, V, K, self._num_processes,
                float(self._cutoff_prob), int(self._cutoff_top_n), int(self._blank_id), self._log_probs,
                output.data_ptr(), timesteps.data_ptr(), scores.data_ptr(), out_len.data_ptr(), nres.data_ptr(), out_T, stream))
            if check or any_eos:
                self._unchecked = 0
                _native.check(_native.lib.ctcd_check_status(self._handle, B))
            else:
                self._unchecked = B  # (peek() looks at these status words with its own)
        if any_eos:
            self._ptr_cache = None  # (ended streams are not decoded again: the next call brings other states)
        if not any_eos:  # nothing ended: no results (binding.cpp:186-205 sizes them to the most results of any item: none)
            return (torch.zeros((B, 0, 0), dtype=torch.int32), torch.zeros((B, K), dtype=torch.float32),
                    torch.zeros((B, 0, 0), dtype=torch.int32), torch.zeros((B, K), dtype=torch.int32))
        nres_c = nres.cpu()
        out_len_c = out_len.cpu()
        R = int(nres_c.max()) if B else 0          # binding.cpp:186-205: sized to the most results / the longest beam
        L = int(out_len_c.max()) if B and R else 0
        return _to_host((output[:, :R, :L].contiguous(), scores, timesteps[:, :R, :L].contiguous(), out_len))

    def greedy_decode_device(self, probs, states, is_eos_s, seq_lens=None, details=False):
        """Greedy (best-path) decoding of live streams on the device (extension; include/ctcdecode_amd.h "Greedy decode of live streams"):
        feeds the chunk ``probs[b, :seq_lens[b]]`` to the ``GreedyState`` ``states[b]`` and returns the labels whose emitting frame lies in
        the chunk -- final labels: best-path decoding never revises one.  However a stream's frames are cut into chunks, its calls return,
        concatenated, what ``CTCBeamDecoder.greedy_decode_device`` returns for all its frames together, bit for bit.

        Returns ``(tokens [B, 1, Tc] int32, scores [B, 1] float32, timesteps [B, 1, Tc] int32, out_lens [B, 1] int32)`` in HBM on the
        decoder's device, asynchronous on the current stream; nothing is read on the host.  ``timesteps`` count frames from the stream's
        ``first_frame``; ``scores`` is the score of all frames so far, this chunk included (0 for a stream that never had a frame).  With
        ``details=True`` three more tensors follow: ``ends`` int32 [B, 1, Tc + 1] and ``label_scores`` float32 [B, 1, Tc + 1] of the runs
        whose last frame became known in this call -- a run that reaches the chunk's last frame of a stream that goes on is reported by
        a later call -- and ``closed_lens`` int32 [B, 1], their count; over a stream's life the i-th closed run is the i-th label's.
        Positions at or beyond a count are 0.

        ``is_eos_s[b]`` ends stream ``b`` with this chunk (an empty chunk too); an ended state raises ``ValueError`` until it is
        ``reset()``.  Follows the decoder's ``blank_id`` and input mode; half dtypes on the device are read as they are.  No language
        model, no ``cutoff_top_n`` / ``cutoff_prob`` and no blank filter take part; the beam streams (``DecoderState``) are untouched."""
        if probs.dim() != 3:
            raise ValueError("probs must be [batch, time, labels]")
        probs = _input_rows(self, probs)
        B, T, V = probs.shape
        if V != self._num_labels:
            raise ValueError("probs.shape[2] (%d) does not match the number of labels (%d)" % (V, self._num_labels))
        if not 0 <= int(self._blank_id) < V:
            raise ValueError("ctcdecode_amd: blank_id must index the vocabulary")
        if len(states) != B or len(is_eos_s) != B:
            raise ValueError("states and is_eos_s need one entry per batch item")
        # (a serving loop calls this once per chunk with the same states: the list is looked at, and the array of handles rebuilt, only
        #  when it changes -- weak references, as in ``decode``; an ended or a duplicate state is refused by the library itself)
        cache = getattr(self, "_greedy_ptr_cache", None)
        if cache is None or len(cache[0]) != B or any(r() is not st for r, st in zip(cache[0], states)):
            if len(set(id(st) for st in states)) != B:
                raise ValueError("the same GreedyState twice in one call")
            for st in states:
                if not isinstance(st, GreedyState):
                    raise ValueError("greedy_decode takes GreedyState objects (DecoderState belongs to decode)")
                if st._device != self._device:
                    raise ValueError("GreedyState of device %s used with a decoder of device %s" % (st._device, self._device))
                if st.ended:
                    raise ValueError("GreedyState has ended: reset() it before it is fed again")
            cache = ([weakref.ref(st) for st in states], (ctypes.c_void_p * max(B, 1))(*[st._handle.value for st in states]))
            self._greedy_ptr_cache = cache
        ptrs = cache[1]
        if seq_lens is not None:
            seq_lens = seq_lens.to(device=self._device, dtype=torch.int32).contiguous()
            if seq_lens.numel() != B:
                raise ValueError("seq_lens must have one entry per batch item")
        any_eos = any(is_eos_s)
        eos = (ctypes.c_ubyte * max(B, 1)).from_buffer_copy(bytes(bytearray(1 if e else 0 for e in is_eos_s)) or b"\0")
        with torch.cuda.device(self._device):
            tokens = torch.empty((B, 1, T), dtype=torch.int32, device=self._device)
            starts = torch.empty((B, 1, T), dtype=torch.int32, device=self._device)
            ends = torch.empty((B, 1, T + 1), dtype=torch.int32, device=self._device) if details else None
            label_scores = torch.empty((B, 1, T + 1), dtype=torch.float32, device=self._device) if details else None
            closed_lens = torch.empty((B, 1), dtype=torch.int32, device=self._device) if details else None
            scores = torch.empty((B, 1), dtype=torch.float32, device=self._device)
            out_lens = torch.empty((B, 1), dtype=torch.int32, device=self._device)
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(_native.lib.ctcd_greedy_stream_decode(
                self._handle, ptrs, eos, probs.data_ptr(), seq_lens.data_ptr() if seq_lens is not None else None, B, T, V, int(self._blank_id),
                self._log_probs, tokens.data_ptr(), starts.data_ptr(), ends.data_ptr() if details else None,
                label_scores.data_ptr() if details else None, closed_lens.data_ptr() if details else None, scores.data_ptr(), out_lens.data_ptr(), stream))
        if any_eos:
            for st, e in zip(states, is_eos_s):
                if e:
                    st._ended = True
            self._greedy_ptr_cache = None  # (ended streams are not fed again: the next call brings other states)
        return (tokens, scores, starts, out_lens, ends, label_scores, closed_lens) if details else (tokens, scores, starts, out_lens)

    def greedy_decode(self, probs, states, is_eos_s, seq_lens=None, details=False):
        """``greedy_decode_device`` with its tensors on the CPU."""
        outs = self.greedy_decode_device(probs, states, is_eos_s, seq_lens, details)
        return tuple(o.cpu() for o in outs) if any(o.numel() == 0 for o in outs) else tuple(_to_host(outs))

    def peek(self, states, n_best=1, since=None):
        """Interim results of live streams (extension; the reference reports nothing before ``is_eos``): what the streams' one-shot
        decode of the frames fed so far returns, without feeding a frame and without disturbing the streams.

        Returns CPU tensors ``beam_results[B, n, L], beam_scores[B, n], timesteps[B, n, L], out_lens[B, n], stable_lens[B]``: n = the
        most results of any stream (at most ``n_best``), ``out_lens`` the FULL lengths, ``beam_results`` / ``timesteps`` the labels
        from depth ``since[b]`` on (``since``: a sequence of B ints or None = 0; L = the longest reported part).  ``stable_lens[b]``
        labels of every row of stream b are final -- every later result of the stream begins with them, time steps included -- so a
        client commits them and asks with ``since=stable_lens`` next time.  Works behind ``decode(..., check=False)`` chunks."""
        B = len(states)
        n_best = int(n_best)
        if n_best < 1:
            raise ValueError("n_best must be at least 1")
        if since is not None and len(since) != B:
            raise ValueError("since needs one entry per stream")
        if self._scorer is not None and isinstance(self._scorer, CallbackScorer):
            raise NotImplementedError("ctcdecode_amd: interim results of streams behind a callback scorer")
        if B == 0:
            return (torch.zeros((0, 0, 0), dtype=torch.int32), torch.zeros((0, 0), dtype=torch.float32), torch.zeros((0, 0, 0), dtype=torch.int32),
                    torch.zeros((0, 0), dtype=torch.int32), torch.zeros((0,), dtype=torch.int32))
        ptrs = (ctypes.c_void_p * B)(*[st._ptr(self) for st in states])
        sin = [max(0, int(v)) for v in since] if since is not None else [0] * B
        # the device buffers are bounded by what the host knows: no row is longer than the frames its stream has been fed
        L_cap = max(0, max(int(_native.lib.ctcd_stream_frames(ptrs[b])) - sin[b] for b in range(B)))
        since_c = (ctypes.c_int32 * B)(*sin)
        with torch.cuda.device(self._device):
            tok = torch.empty((B, n_best, L_cap), dtype=torch.int32, device=self._device)
            ts = torch.empty((B, n_best, L_cap), dtype=torch.int32, device=self._device)
            scores = torch.empty((B, n_best), dtype=torch.float32, device=self._device)
            # [out_lens | n_results | stable_lens]: one small copy tells the host how much of the label tensors to bring over
            meta = torch.empty((B * (n_best + 2),), dtype=torch.int32, device=self._device)
            out_len, nres, stable = meta[:B * n_best].view(B, n_best), meta[B * n_best:B * n_best + B], meta[B * n_best + B:]
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(_native.lib.ctcd_stream_peek(self._handle, ptrs, B, n_best, since_c, tok.data_ptr(), ts.data_ptr(), L_cap,
                                                       scores.data_ptr(), out_len.data_ptr(), nres.data_ptr(), stable.data_ptr(), stream))
            unchecked, self._unchecked = getattr(self, "_unchecked", 0), 0
            _native.check(_native.lib.ctcd_check_status(self._handle, unchecked))
            meta_c = meta.cpu()
            out_len_c = meta_c[:B * n_best].view(B, n_best)
            n = int(meta_c[B * n_best:B * n_best + B].max())
            rep = out_len_c[:, :n] - torch.tensor(sin, dtype=torch.int32).view(B, 1)
            L = max(0, int(rep.max())) if n else 0
            return (tok[:, :n, :L].cpu(), scores[:, :n].cpu(), ts[:, :n, :L].cpu(), out_len_c[:, :n].contiguous(), meta_c[B * n_best + B:].contiguous())

    def compact(self, states):
        """Give back the memory of live streams (extension; the reference frees trie nodes as it goes): every stream keeps exactly
        the trie nodes its current beam can still reach and drops the rest of its node pool.  Nothing a later ``decode`` or ``peek``
        returns changes, however often and wherever between chunks this is called.  Returns the nodes kept per stream (a list of B
        ints).  A stream that now needs at most a quarter of its block moves to a smaller one (``DecoderState.nbytes`` falls).
        Works behind ``decode(..., check=False)`` chunks; synchronous."""
        B = len(states)
        if B == 0:
            return []
        ptrs = (ctypes.c_void_p * B)(*[st._ptr(self) for st in states])
        live = (ctypes.c_int32 * B)()
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            self._check(_native.lib.ctcd_stream_compact(self._handle, ptrs, B, live, stream))
            # (the call has waited for the chunks queued in front of it: their status words are looked at now, as peek() does)
            unchecked, self._unchecked = getattr(self, "_unchecked", 0), 0
            _native.check(_native.lib.ctcd_check_status(self._handle, unchecked))
        return [int(v) for v in live]

    def commit(self, states):
        """Hand out the final labels of live streams and drop them from the streams (extension): of the ``stable_lens`` labels every
        hypothesis of a stream shares (see ``peek``), all but the last are returned -- once -- and their trie nodes leave the node
        pool together with the dead ones (see ``compact``).  Returns a list of ``(tokens, timesteps)`` int32 CPU tensors, one pair
        per stream: the labels committed by THIS call with their absolute time steps; the caller keeps the transcript, the library
        does not.  From then on ``peek`` (lengths, ``since``, ``stable_lens``) and the stream-ending ``decode`` report every row
        without its first ``DecoderState.committed_len`` labels: committed ++ reported row is the reference's row, scores and row
        order unchanged.  A stream with nothing new to commit is compacted.  Works behind ``decode(..., check=False)`` chunks;
        synchronous.  Streams with a scorer raise ``NotImplementedError`` (their scores use a prefix's absolute length)."""
        B = len(states)
        if B == 0:
            return []
        ptrs = (ctypes.c_void_p * B)(*[st._ptr(self) for st in states])
        counts = (ctypes.c_int32 * B)()
        made = {}

        def alloc(_user, _R, L, p_tok, p_ts):
            try:
                made["tok"] = torch.zeros((B, L), dtype=torch.int32)
                made["ts"] = torch.zeros((B, L), dtype=torch.int32)
                p_tok[0] = made["tok"].data_ptr()
                p_ts[0] = made["ts"].data_ptr()
                return 0
            except Exception as e:  # (reported through the return code: no exception crosses the C frame)
                made["error"] = e
                return 1

        cb = _native.RESULT_ALLOC_FN(alloc)
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            rc = _native.lib.ctcd_stream_commit(self._handle, ptrs, B, cb, None, counts, None, None, stream)
            if "error" in made:
                raise made["error"]
            self._check(rc)
            # (the call has waited for the chunks queued in front of it: their status words are looked at now, as peek() does)
            unchecked, self._unchecked = getattr(self, "_unchecked", 0), 0
            _native.check(_native.lib.ctcd_check_status(self._handle, unchecked))
        # (rows of the two [B, L] tensors the allocator made; a stream that committed nothing gets the one pair of empty tensors)
        none = (made["tok"][0, :0], made["ts"][0, :0])
        if made["tok"].shape[1] == 0:
            return [none] * B
        rows_tok, rows_ts = made["tok"].unbind(0), made["ts"].unbind(0)
        return [(rows_tok[b][:n], rows_ts[b][:n]) if n else none for b, n in enumerate(counts)]

    def save(self, states):
        """Images of live streams in host memory (extension): one 1-D ``torch.uint8`` CPU tensor per stream -- views of one allocation
        -- that holds everything the stream is: ``restore`` on this decoder, on another one with the same labels, beam width and blank
        (another kernel choice, another GPU, another process) gives a stream that behaves bit-identically from then on, for every
        later ``decode``, ``peek``, ``compact``, ``commit`` and stream end.  ``committed_len``, the absolute frame numbers and the
        scorer's fingerprint travel; the committed labels themselves are the caller's (see ``commit``).

        ``save`` has exactly ``compact(states)``'s effect on the saved streams -- an image is the layout a compaction leaves, and a
        compaction changes nothing a later call returns -- and changes nothing else about them: they stay live and decode on.  The
        image is canonical (saving twice with no frame in between gives identical bytes) and small: 4 * (28 + A * beam + 5 * M)
        bytes for the M trie nodes the beam can still reach, A = 14 without a scorer and 26 with one.  Works behind
        ``decode(..., check=False)`` chunks; synchronous.  Streams behind a callback scorer raise ``NotImplementedError`` (their
        states index a per-process cache) and are left untouched."""
        B = len(states)
        if B == 0:
            return []
        if self._scorer is not None and isinstance(self._scorer, CallbackScorer):
            raise NotImplementedError("ctcdecode_amd: images of streams behind a callback scorer")
        if self._blank_skip is not None:
            raise NotImplementedError("ctcdecode_amd: images of streams that decode behind blank_skip (an image does not hold the frame map)")
        ptrs = (ctypes.c_void_p * B)(*[st._ptr(self) for st in states])
        sizes = (ctypes.c_ulonglong * B)()
        made = {}

        def alloc(_user, total):
            try:
                made["buf"] = torch.empty((int(total),), dtype=torch.uint8, pin_memory=int(total) > 0)  # (every byte is written)
                return made["buf"].data_ptr()
            except Exception as e:  # (reported through the return value: no exception crosses the C frame)
                made["error"] = e
                return None

        cb = _native.BYTES_ALLOC_FN(alloc)
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            rc = _native.lib.ctcd_stream_save(self._handle, ptrs, B, cb, None, sizes, stream)
            if "error" in made:
                raise made["error"]
            self._check(rc)
            # (the call has waited for the chunks queued in front of it: their status words are looked at now, as peek() does)
            unchecked, self._unchecked = getattr(self, "_unchecked", 0), 0
            _native.check(_native.lib.ctcd_check_status(self._handle, unchecked))
        out, at = [], 0
        for n in sizes:  # (image b starts at the sum of the earlier sizes, each rounded up to 16 bytes)
            out.append(made["buf"][at:at + int(n)])
            at += (int(n) + 15) // 16 * 16
        return out

    def restore(self, blobs, frames_hint=0):
        """New ``DecoderState`` objects, bound to this decoder, from images ``save`` made (uint8 tensors or ``bytes``) -- on this
        decoder or on any other with the same labels, beam width and blank, and a scorer built from the same model if the streams had
        one.  Every image is validated on the host before anything is allocated or uploaded; an image that is truncated, corrupted,
        of another beam width / label count or saved behind another scorer raises ``ValueError`` naming the item and the check, and
        then no stream is created.  ``frames_hint``: the capacity the streams start with (as for a new ``DecoderState``)."""
        B = len(blobs)
        if B == 0:
            return []
        if self._scorer is not None and isinstance(self._scorer, CallbackScorer):
            raise NotImplementedError("ctcdecode_amd: images of streams behind a callback scorer")
        if self._blank_skip is not None:
            raise NotImplementedError("ctcdecode_amd: restore on a decoder with blank_skip (an image does not hold the frame map)")
        keep = []
        for b, blob in enumerate(blobs):
            if isinstance(blob, torch.Tensor):
                if blob.dtype != torch.uint8 or blob.dim() != 1:
                    raise ValueError("restore: item %d is not a 1-D uint8 tensor" % b)
                t = blob.detach().cpu().contiguous()
            else:
                t = torch.frombuffer(bytearray(bytes(blob)), dtype=torch.uint8) if len(blob) else torch.zeros((0,), dtype=torch.uint8)
            keep.append(t)
            try:
                inf = snapshot_info(t)
            except ValueError as e:
                raise ValueError("restore: item %d is refused: %s" % (b, e))
            if inf["beam"] != self._beam_width or inf["labels"] != self._num_labels:
                raise ValueError("restore: item %d was saved with beam width %d over %d labels; this decoder has %d over %d"
                                 % (b, inf["beam"], inf["labels"], self._beam_width, self._num_labels))
        ptrs = (ctypes.c_void_p * B)(*[t.data_ptr() for t in keep])
        sizes = (ctypes.c_ulonglong * B)(*[t.numel() for t in keep])
        outs = (ctypes.c_void_p * B)()
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            self._check(_native.lib.ctcd_stream_restore(self._handle, self._scorer.handle if self._scorer is not None else None, ptrs, sizes, B,
                                                        int(frames_hint), outs, stream))
        return [DecoderState._adopt(self, outs[b]) for b in range(B)]

    def character_based(self):
        return bool(_native.lib.ctcd_scorer_is_character_based(self._scorer.handle)) if self._scorer else None

    def max_order(self):
        return int(_native.lib.ctcd_scorer_max_order(self._scorer.handle)) if self._scorer else None

    def dict_size(self):
        return int(_native.lib.ctcd_scorer_dict_size(self._scorer.handle)) if self._scorer else None

    def reset_params(self, alpha, beta):
        if self._scorer is not None:
            _native.check(_native.lib.ctcd_scorer_reset_params(self._scorer.handle, float(alpha), float(beta)))

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                _native.destroy(_native.lib.ctcd_destroy, h)
            except Exception:
                pass
            self._handle = None


def snapshot_info(blob):
    """What an image made by ``OnlineCTCBeamDecoder.save`` says about itself (a uint8 tensor or ``bytes``), without a GPU: a dict with
    ``version, beam, labels, frames, committed, nodes, scorer_kind`` (0 none / 1 built-in), ``fingerprint`` and ``bytes``.
    ``ValueError``: not an image."""
    if isinstance(blob, torch.Tensor):
        t = blob.detach().cpu().contiguous().view(torch.uint8).reshape(-1)
        ptr, n = t.data_ptr(), t.numel()
    else:
        t = bytes(blob)
        ptr, n = ctypes.cast(ctypes.c_char_p(t), ctypes.c_void_p), len(t)
    info = _native.SnapshotInfo()
    _native.check(_native.lib.ctcd_snapshot_info(ptr if n else None, n, ctypes.byref(info)))
    return dict((k, int(getattr(info, k))) for k in ("version", "beam", "labels", "frames", "committed", "nodes", "scorer_kind", "fingerprint", "bytes"))


class DecoderState(object):
    """State of one audio stream (ctcdecode/__init__.py:253-272).  Bound to the decoder it is first used with; not reusable
    after its stream ended, as in the reference."""

    def __init__(self, decoder):
        self._decoder = decoder
        h = ctypes.c_void_p()
        sc = getattr(decoder, "_scorer", None)  # ctcdecode/__init__.py:255-269: the state is created with the decoder's scorer
        _native.check(_native.lib.ctcd_stream_create_lm(decoder._handle, ctypes.byref(h), decoder._num_labels, decoder._beam_width, 0,
                                                        sc.handle if sc is not None else None))
        self.state = h

    @classmethod
    def _adopt(cls, decoder, handle):
        """A DecoderState around a stream handle the library made (``OnlineCTCBeamDecoder.restore``); it owns the handle from here on."""
        self = cls.__new__(cls)
        self._decoder = decoder
        self.state = ctypes.c_void_p(handle)
        return self

    def _ptr(self, decoder):
        if decoder is not self._decoder:
            raise ValueError("DecoderState used with a different decoder than it was created for")
        return self.state.value

    @property
    def frames(self):
        """Frames the stream has been fed so far."""
        return int(_native.lib.ctcd_stream_frames(self.state))

    @property
    def frames_seen(self):
        """Frames the stream has been fed so far.  Behind ``OnlineCTCBeamDecoder.set_blank_skip`` ``frames`` counts the frames decoded
        -- the kept ones -- and this the frames the filter has looked at; elsewhere the two are equal."""
        return int(_native.lib.ctcd_stream_frames_seen(self.state))

    @property
    def nbytes(self):
        """Bytes of HBM the stream's block holds now (it doubles as the stream grows; ``OnlineCTCBeamDecoder.compact`` can shrink it)."""
        return int(_native.lib.ctcd_stream_bytes(self.state))

    @property
    def committed_len(self):
        """Labels ``OnlineCTCBeamDecoder.commit`` has handed out for this stream so far: what it reports now counts from there."""
        return int(_native.lib.ctcd_stream_committed(self.state))

    @property
    def pool_nodes(self):
        """Upper bound of the trie nodes in the stream's pool: frames * beam + 1, or nodes kept + (frames since) * beam after a compaction."""
        return int(_native.lib.ctcd_stream_pool_nodes(self.state))

    def __del__(self):
        h = getattr(self, "state", None)
        d = getattr(self, "_decoder", None)
        if h is not None and h.value and d is not None and getattr(d, "_handle", None) is not None:
            try:
                _native.destroy(_native.lib.ctcd_stream_destroy, d._handle, h)
            except Exception:
                pass
            self.state = None


class GreedyState(object):
    """State of one audio stream under greedy (best-path) decoding (extension; ``OnlineCTCBeamDecoder.greedy_decode`` /
    ``greedy_decode_device``): 32 bytes on the decoder's device -- the frames fed, the last frame's label, the open run's maximum, the
    running score, the counts.  ``first_frame``: the number reported for the stream's first frame (``timesteps`` and ``ends`` count from
    it); a stream's frame numbers stay below 2**31 - 1 (``NotImplementedError`` from the call that would pass it).  Not reusable after
    its stream ended, until ``reset()``."""

    def __init__(self, decoder, first_frame=0):
        self._decoder = decoder
        self._device = decoder._device
        self._ended = False
        h = ctypes.c_void_p()
        _native.check(_native.lib.ctcd_greedy_stream_create(decoder._handle, ctypes.byref(h), int(first_frame)))
        self._handle = h

    def reset(self, first_frame=0):
        """A fresh stream again (queued on the current stream of the state's device)."""
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream(self._device).cuda_stream
            _native.check(_native.lib.ctcd_greedy_stream_reset(self._decoder._handle, self._handle, int(first_frame), stream))
        self._ended = False

    @property
    def ended(self):
        """True once a call has fed the stream with ``is_eos`` set."""
        return self._ended

    def info(self):
        """Waits for the device: ``dict(frames, emitted, closed, open_run)`` -- frames fed, labels emitted, runs closed so far, and
        whether a run is open (its label emitted, its last frame not yet known)."""
        out = (ctypes.c_longlong * 4)()
        _native.check(_native.lib.ctcd_greedy_stream_info(self._decoder._handle, self._handle, out))
        return dict(frames=int(out[0]), emitted=int(out[1]), closed=int(out[2]), open_run=bool(out[3]))

    def __del__(self):
        h = getattr(self, "_handle", None)
        d = getattr(self, "_decoder", None)
        if h is not None and h.value and d is not None and getattr(d, "_handle", None) is not None:
            try:
                _native.destroy(_native.lib.ctcd_greedy_stream_destroy, d._handle, h)
            except Exception:
                pass
            self._handle = None
