"""A stand-in for the `kenlm` Python module over the built-in ARPA tables, for testing KenlmScorer where kenlm is not installed.

It is deliberately NOT importable as `kenlm` (tests/test_gpu_lm.py skips its kenlm test when that import fails): tests put it in
place with ``monkeypatch.setitem(sys.modules, "kenlm", fake_kenlm.module(...))``.

``module(cond_log10, vocabulary, order)`` builds the module object.  ``cond_log10(words)`` answers one window (tuple of str, oldest
first) with kenlm's float32 log10 probability, or None when a word is unknown:
  * ``restated_backend`` (CPU): tests/oracle_util.py's restated scorer.  Its ``cond_logprob`` returns the reference's converted value,
    log10 / NUM_FLT_LOGE, as a double; the float32 log10 is recovered exactly by multiplying back and rounding to float32 (the
    division and the multiplication each err by at most half a double ulp, far below half a float32 ulp).
  * ``library_backend`` (GPU): ``ctcd_scorer_cond_log10`` of a built-in scorer of the library.
Like kenlm, a ``State`` carries at most ``order - 1`` words of history: ``BaseScore(state, word, out)`` scores ``word`` after
``state``'s words and leaves the last ``order - 1`` words of the window in ``out``.
"""
import ctypes
import types

import numpy as np

NUM_FLT_LOGE = float(np.float32(0.4342944819))


class _State(object):
    __slots__ = ("words",)

    def __init__(self):
        self.words = ()


def module(cond_log10, vocabulary, order):
    vocab = frozenset(vocabulary) | {"<s>", "</s>"}

    class Model(object):
        def __init__(self, path):
            self.path = str(path)
            self.order = int(order)

        def __contains__(self, word):
            return word in vocab

        def NullContextWrite(self, state):
            state.words = ()

        def BeginSentenceWrite(self, state):
            state.words = ("<s>",)

        def BaseScore(self, state, word, out):
            window = state.words + (word,)
            p = cond_log10(window)
            out.words = window[-(self.order - 1):] if self.order > 1 else ()
            return -100.0 if p is None else p  # (kenlm scores an unknown word with <unk>; KenlmScorer never asks one)

    m = types.ModuleType("kenlm")
    m.Model = Model
    m.State = _State
    return m


def arpa_words(path):
    """The unigrams of an ARPA file."""
    words, on = [], False
    with open(path, encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if line.startswith("\\"):
                on = line == "\\1-grams:"
                continue
            if on and line:
                words.append(line.split("\t")[1] if "\t" in line else line.split()[1])
    return words


def restated_backend(scorer):
    """cond_log10 over an oracle_util.Scorer (the restated checker): float32 log10, None for an unknown word."""

    def cond_log10(words):
        v = scorer.cond_logprob(list(words))
        return None if v == -1000.0 else float(np.float32(v * NUM_FLT_LOGE))

    return cond_log10


def library_backend(lib, handle):
    """cond_log10 over ctcd_scorer_cond_log10 of a library scorer (lib: ctcdecode_amd._native.lib)."""

    def cond_log10(words):
        arr = (ctypes.c_char_p * len(words))(*[w.encode("utf-8") for w in words])
        p = ctypes.c_float()
        rc = lib.ctcd_scorer_cond_log10(handle, arr, len(words), ctypes.byref(p))
        if rc < 0:
            raise RuntimeError("ctcd_scorer_cond_log10 failed")
        return None if rc else p.value

    return cond_log10
