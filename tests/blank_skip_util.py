"""Helpers of the blank-frame filter's tests (TEST INFRASTRUCTURE ONLY): the definition of ``CTCBeamDecoder(blank_skip=thr)`` restated
in numpy -- filter, the oracle's decode of the kept rows, the time steps mapped back -- the case table both test files share, and the
ctypes front-end of the host twin (tests/native/blank_skip_host.cpp)."""
import ctypes
import math
import os

import numpy as np
import oracle_util as ou

ROOT = ou.ROOT
NATIVE = os.path.join(ROOT, "tests", "native")
SKIP_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcskip_host.so")
DTYPES = {"f32": 0, "f16": 1, "bf16": 2}

_i32p = ctypes.POINTER(ctypes.c_int32)


def which_oracle():
    return "reference" if ou.have_reference() else "restated"


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def bound(thr, mode):
    """The float32 the blank's value is compared with: mode "prob" -> thr, "log" / "logits" -> log(thr)."""
    return np.float32(thr) if mode == "prob" else np.float32(math.log(thr))


def blank_values(x, blank_id, mode):
    """float32 [B, T]: what the definition compares -- the blank's entry of every frame, widened exactly; raw logits: of the product's
    float32 log-softmax of that row (the host twin of ctcd_log_softmax)."""
    x = np.asarray(x)
    if mode == "logits":
        x = ou.log_softmax_rows(x.astype(np.float32))
    return x[:, :, blank_id].astype(np.float32)


def filter_frames(x, seq_lens, blank_id, thr, mode):
    """-> (kept int32 [B, T] with a zero tail, n' int32 [B]).  Skipped iff v > c, ordered and strict; frames at or beyond n are not
    looked at."""
    B, T = x.shape[:2]
    v = blank_values(x, blank_id, mode)
    c = bound(thr, mode)
    kept = np.zeros((B, T), np.int32)
    n2 = np.zeros((B,), np.int32)
    for b in range(B):
        n = T if seq_lens is None else min(max(int(seq_lens[b]), 0), T)
        with np.errstate(invalid="ignore"):
            idx = np.nonzero(~(v[b, :n] > c))[0]
        kept[b, :len(idx)] = idx
        n2[b] = len(idx)
    return kept, n2


def gather_rows(x, kept, n2):
    """The kept rows, densely; rows at or beyond n' are zero here (the product leaves them unspecified)."""
    out = np.zeros_like(x)
    for b in range(x.shape[0]):
        out[b, :n2[b]] = x[b, kept[b, :n2[b]]]
    return out


def remap(res, kept):
    """The oracle's result dict with every reported time step s replaced by kept[b, s] (valid prefixes only)."""
    out = {k: v.copy() for k, v in res.items()}
    B, K = res["lens"].shape
    for b in range(B):
        for p in range(K):
            L = int(res["lens"][b, p])
            out["timesteps"][b, p, :L] = kept[b, res["timesteps"][b, p, :L]]
    return out


def decode(x, seq_lens, thr, mode="log", blank_id=0, scorer=None, which=None, **kw):
    """The contract: the oracle on the kept rows with seq_lens = n', time steps mapped back.  ``x`` float32 / float16 values (a half
    input is widened exactly first); mode "prob" | "log" | "logits".  -> (result dict, kept, n')."""
    which = which or which_oracle()
    x32 = np.asarray(x).astype(np.float32)
    kept, n2 = filter_frames(x32, seq_lens, blank_id, thr, mode)
    rows = ou.log_softmax_rows(x32) if mode == "logits" else x32
    res = ou.decode(gather_rows(rows, kept, n2), n2, blank_id=blank_id, log_input=mode != "prob", which=which, scorer=scorer, **kw)
    return remap(res, kept), kept, n2


def plain(x, seq_lens, mode="log", blank_id=0, scorer=None, which=None, **kw):
    """The unfiltered decode of the same oracle."""
    x32 = np.asarray(x).astype(np.float32)
    rows = ou.log_softmax_rows(x32) if mode == "logits" else x32
    return ou.decode(rows, None if seq_lens is None else np.asarray(seq_lens, np.int32), blank_id=blank_id, log_input=mode != "prob",
                     which=which or which_oracle(), scorer=scorer, **kw)


# ---- the case table ----------------------------------------------------------------------------------------------------------------
ANCHOR = dict(B=4, T=150, V=29, seed=11, blank_bias=4.0, seq_lens=[150, 97, 0, 64], thr=0.6, beam=8)
_CACHE = {}


def anchor_input():
    a = ANCHOR
    return ou.synth_logprobs(a["B"], a["T"], a["V"], a["seed"], blank_bias=a["blank_bias"]), np.asarray(a["seq_lens"], np.int32)


def anchor_want():
    """(result, kept, n') of the anchor case: computed once, shared, never written to."""
    if "anchor" not in _CACHE:
        lp, sl = anchor_input()
        _CACHE["anchor"] = decode(lp, sl, ANCHOR["thr"], beam=ANCHOR["beam"])
    return _CACHE["anchor"]


def synth(B, T, V, seed, blank_bias=4.0, blank_id=0, mode="log"):
    """Log-probabilities with a biased blank; mode "prob": their exponentials; "logits": the unnormalised rows (a constant per frame
    added, so that the log-softmax has work to do)."""
    lp = ou.synth_logprobs(B, T, V, seed, blank_bias=blank_bias, blank_id=blank_id)
    if mode == "prob":
        return np.exp(lp).astype(np.float32)
    if mode == "logits":
        shift = np.random.default_rng(seed + 1).standard_normal((B, T, 1)).astype(np.float32) * np.float32(3)
        return (lp + shift).astype(np.float32)
    return lp


def to_dtype_values(x, dtype):
    """``x`` rounded to the dtype's values, as float32 (what the device widens a half tensor to)."""
    if dtype == "f32":
        return x.astype(np.float32)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    u = x.astype(np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint32) << np.uint32(16)  # round to nearest even
    return r.view(np.float32)


def to_dtype_bits(x32, dtype):
    """The storage of values that are exactly representable in ``dtype``: float32 array, or uint16 patterns."""
    if dtype == "f32":
        return np.ascontiguousarray(x32, np.float32)
    if dtype == "f16":
        return np.ascontiguousarray(x32.astype(np.float16)).view(np.uint16)
    return np.ascontiguousarray((x32.view(np.uint32) >> np.uint32(16)).astype(np.uint16))


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_skip_host():
    import subprocess

    src = os.path.join(NATIVE, "blank_skip_host.cpp")
    deps = [src, os.path.join(ROOT, "ctcdecode_amd", "csrc", "blank_skip.h")]
    if os.path.exists(SKIP_HOST_SO) and all(os.path.getmtime(SKIP_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return SKIP_HOST_SO
    os.makedirs(os.path.dirname(SKIP_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (SKIP_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, SKIP_HOST_SO)
    return SKIP_HOST_SO


def _lib():
    lib = ctypes.CDLL(build_skip_host())
    lib.ctcskip_host_filter.argtypes = [ctypes.c_void_p, ctypes.c_int, _i32p] + [ctypes.c_int] * 4 + [ctypes.c_float, ctypes.c_void_p, _i32p, _i32p]
    lib.ctcskip_host_remap_timesteps.argtypes = [_i32p] * 4 + [ctypes.c_int] * 3
    lib.ctcskip_host_remap_timesteps.restype = None
    lib.ctcskip_host_remap_compact.argtypes = [_i32p, _i32p, ctypes.POINTER(ctypes.c_uint32), _i32p, _i32p] + [ctypes.c_int] * 3
    lib.ctcskip_host_remap_compact.restype = None
    lib.ctcskip_host_widen_bits.argtypes = [ctypes.c_int, ctypes.c_uint16]
    lib.ctcskip_host_widen_bits.restype = ctypes.c_uint32
    lib.ctcskip_host_tile_rows.argtypes = [ctypes.c_longlong]
    return lib


def host_filter(bits, dtype, seq_lens, blank_id, c, fill=0x5A):
    """The twin's filter on the storage ``bits`` ([B, T, V] float32 or uint16).  -> (rows as written over a buffer of ``fill`` bytes,
    n', kept, word size of the gather)."""
    B, T, V = bits.shape
    out = np.frombuffer(bytes([fill]) * bits.nbytes, dtype=bits.dtype).reshape(bits.shape).copy()
    n2 = np.full((B,), -1, np.int32)
    kept = np.full((B, T), -1, np.int32)
    sl = None if seq_lens is None else np.ascontiguousarray(seq_lens, np.int32)
    w = _lib().ctcskip_host_filter(bits.ctypes.data, DTYPES[dtype], None if sl is None else sl.ctypes.data_as(_i32p), B, T, V, int(blank_id), float(c),
                                   out.ctypes.data, n2.ctypes.data_as(_i32p), kept.ctypes.data_as(_i32p))
    assert w > 0, "the twin refused its arguments"
    return out, n2, kept, w


def host_remap_timesteps(timesteps, lens, kept, n2):
    ts = np.ascontiguousarray(timesteps, np.int32).copy()
    B, K, T = ts.shape
    ln, kp, kl = (np.ascontiguousarray(a, np.int32) for a in (lens, kept, n2))
    _lib().ctcskip_host_remap_timesteps(ts.ctypes.data_as(_i32p), ln.ctypes.data_as(_i32p), kp.ctypes.data_as(_i32p), kl.ctypes.data_as(_i32p), B, K, T)
    return ts


def compact_of(res, b_items=None):
    """A result dict in compact form, every entry owning its whole row (shares nothing with its predecessor): (hdr [B,4], ent [B,K,4],
    labels uint32 [n]) with records label | frame << 16 -- a valid, if wasteful, instance of the format."""
    B, K = res["lens"].shape
    hdr = np.zeros((B, 4), np.int32)
    ent = np.zeros((B, K, 4), np.int32)
    lab = []
    for b in range(B):
        first = len(lab)
        nres = int(res["nres"][b])
        for j in range(nres):
            L = int(res["lens"][b, j])
            ent[b, j] = (j, 0, L, len(lab))
            lab.extend((int(t) | (int(s) << 16)) for t, s in zip(res["tokens"][b, j, :L], res["timesteps"][b, j, :L]))
        hdr[b] = (nres, len(lab) - first, first, 0)
    return hdr, ent, np.asarray(lab, np.uint32)


def host_remap_compact(hdr, ent, labels, kept, n2, T):
    lab = np.ascontiguousarray(labels, np.uint32).copy()
    if lab.size == 0:
        return lab
    B, K = ent.shape[:2]
    kp, kl = np.ascontiguousarray(kept, np.int32), np.ascontiguousarray(n2, np.int32)
    _lib().ctcskip_host_remap_compact(hdr.ctypes.data_as(_i32p), ent.ctypes.data_as(_i32p), lab.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                      kp.ctypes.data_as(_i32p), kl.ctypes.data_as(_i32p), B, K, T)
    return lab


def assert_root_only(got, b, what=""):
    """The zero-frame result of utterance b: the root alone (one result of length 0), everything else zero."""
    assert int(got["lens"][b, 0]) == 0 and not got["tokens"][b].any() and not got["timesteps"][b].any(), what
