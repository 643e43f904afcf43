"""Helpers of the n-best tests (TEST INFRASTRUCTURE ONLY): compact records built in Python from result rows, the contract of
``n_best`` restated on the oracle's tensors, and the ctypes front-end of the host twin (tests/native/nbest_host.cpp)."""
import ctypes
import os

import numpy as np
import oracle_util as ou

ROOT = ou.ROOT
NATIVE = os.path.join(ROOT, "tests", "native")
NBEST_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcnbest_host.so")
BAD_RECORD = 7  # include/ctcdecode_amd.h CTCD_NBEST_BAD_RECORD

_i32p = ctypes.POINTER(ctypes.c_int32)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u8p = ctypes.POINTER(ctypes.c_uint8)


def which_oracle():
    return "reference" if ou.have_reference() else "restated"


# ---- the contract ------------------------------------------------------------------------------------------------------------------
def want_nbest(res, n):
    """The oracle's result dict restricted to rows [:, :n] and defined everywhere: zero beyond a row's length, rows at or beyond the
    item's result count have length 0, score 0 and zero labels.  ``nres`` counts the rows below n that have a result."""
    B, K, T = res["tokens"].shape
    out = dict(tokens=np.zeros((B, n, T), np.int32), timesteps=np.zeros((B, n, T), np.int32), scores=np.zeros((B, n), np.float32),
               lens=np.zeros((B, n), np.int32), nres=np.minimum(res["nres"], n).astype(np.int32))
    for b in range(B):
        for p in range(int(out["nres"][b])):
            L = int(res["lens"][b, p])
            out["tokens"][b, p, :L] = res["tokens"][b, p, :L]
            out["timesteps"][b, p, :L] = res["timesteps"][b, p, :L]
            out["lens"][b, p] = L
            out["scores"][b, p] = res["scores"][b, p]
    return out


def as_dict(output, scores, timesteps, out_lens, want):
    """The four tensors of a product call as a result dict (``nres`` taken from ``want``: the product's tensors do not carry it)."""
    return dict(tokens=np.ascontiguousarray(output.cpu().numpy()), timesteps=np.ascontiguousarray(timesteps.cpu().numpy()),
                scores=np.ascontiguousarray(scores.cpu().numpy()), lens=np.ascontiguousarray(out_lens.cpu().numpy()), nres=want["nres"].copy())


def assert_nbest(got, want, what=""):
    """``got`` against ``want_nbest``: shapes, the defined region bit for bit (oracle_util.assert_same), then the zero fill."""
    for k in ("tokens", "timesteps", "scores", "lens"):
        assert got[k].shape == want[k].shape, "%s: %s has shape %s, want %s" % (what, k, got[k].shape, want[k].shape)
    ou.assert_same(got, want, what)
    assert_zero_fill(got, want["nres"], what)


def assert_zero_fill(got, nres, what=""):
    B, n, T = got["tokens"].shape
    for b in range(B):
        r = int(nres[b])
        assert not got["lens"][b, r:].any(), "%s: item %d: a row without a result has a length" % (what, b)
        assert not got["scores"][b, r:].view(np.uint32).any(), "%s: item %d: a row without a result has a score" % (what, b)
        for p in range(n):
            L = int(got["lens"][b, p])
            assert not got["tokens"][b, p, L:].any(), "%s: item %d row %d: labels beyond the row's length" % (what, b, p)
            assert not got["timesteps"][b, p, L:].any(), "%s: item %d row %d: time steps beyond the row's length" % (what, b, p)


# ---- compact records from result rows ------------------------------------------------------------------------------------------------
def _pairs(res, b, p):
    L = int(res["lens"][b, p])
    return [(int(t) & 0xFFFF) | ((int(s) & 0xFFFF) << 16) for t, s in zip(res["tokens"][b, p, :L], res["timesteps"][b, p, :L])]


def records_of(res, order="trie", share="all", pad=0):
    """A result dict in compact form: (hdr [B,4], ent [B,K,4], labels uint32 [n]).  Every order of the rows is a valid instance as long
    as an entry's first lcp labels equal its predecessor's; ``order``: "trie" (the rows sorted by their label records: the most sharing),
    "reverse" (that order backwards) or "row" (result-row order); ``share``: "all" = lcp is the whole common prefix, "half" = half of
    it (an entry may own labels it could have shared).  ``pad``: unrelated words in front of every item's labels."""
    B, K = res["lens"].shape
    hdr = np.zeros((B, 4), np.int32)
    ent = np.zeros((B, K, 4), np.int32)
    lab = []
    for b in range(B):
        lab.extend([0xDEAD0000 + i for i in range(pad)])
        first = len(lab)
        nres = int(res["nres"][b])
        seqs = [(_pairs(res, b, p), p) for p in range(nres)]
        if order != "row":
            seqs.sort(reverse=order == "reverse")
        prev = []
        for j, (seq, p) in enumerate(seqs):
            lcp = 0
            while lcp < len(seq) and lcp < len(prev) and seq[lcp] == prev[lcp]:
                lcp += 1
            if share == "half":
                lcp //= 2
            if j == 0:
                lcp = 0
            ent[b, j] = (p, lcp, len(seq), len(lab))
            lab.extend(seq[lcp:])
            prev = seq
        hdr[b] = (nres, len(lab) - first, first, 0)
    return hdr, ent, np.asarray(lab, np.uint32)


def trie(entries, K=None):
    """A hand-made item: entries = [(row, lcp, own labels as (token, frame) pairs)] in trie order -> (hdr [1,4], ent [1,K,4], labels)."""
    K = K or len(entries)
    hdr = np.zeros((1, 4), np.int32)
    ent = np.zeros((1, K, 4), np.int32)
    lab = []
    for j, (row, lcp, own) in enumerate(entries):
        ent[0, j] = (row, lcp, lcp + len(own), len(lab))
        lab.extend(int(t) | (int(s) << 16) for t, s in own)
    hdr[0] = (len(entries), len(lab), 0, 0)
    return hdr, ent, np.asarray(lab, np.uint32)


def expand_py(hdr, ent, lab, T):
    """The definition, in Python: label q of entry j is held by the nearest entry o <= j with lcp[o] <= q.  -> result dict with
    tokens / timesteps [B, K, T], lens [B, K], nres [B] (scores zero)."""
    B, K = ent.shape[:2]
    res = dict(tokens=np.zeros((B, K, T), np.int32), timesteps=np.zeros((B, K, T), np.int32), scores=np.zeros((B, K), np.float32),
               lens=np.zeros((B, K), np.int32), nres=hdr[:, 0].astype(np.int32).copy())
    for b in range(B):
        for j in range(int(hdr[b, 0])):
            row, _, dep, _ = (int(v) for v in ent[b, j])
            res["lens"][b, row] = dep
            for q in range(dep):
                o = j
                while o > 0 and int(ent[b, o, 1]) > q:
                    o -= 1
                v = int(lab[int(ent[b, o, 3]) + q - (int(ent[b, o, 1]) if o else 0)])
                res["tokens"][b, row, q] = v & 0xFFFF
                res["timesteps"][b, row, q] = v >> 16
    return res


# ---- the host twin -------------------------------------------------------------------------------------------------------------------
def build_nbest_host():
    import subprocess

    src = os.path.join(NATIVE, "nbest_host.cpp")
    deps = [src] + [os.path.join(ROOT, "ctcdecode_amd", "csrc", f) for f in ("nbest.h", "compact_results.h")]
    if os.path.exists(NBEST_HOST_SO) and all(os.path.getmtime(NBEST_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return NBEST_HOST_SO
    os.makedirs(os.path.dirname(NBEST_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (NBEST_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, NBEST_HOST_SO)
    return NBEST_HOST_SO


def _lib():
    lib = ctypes.CDLL(build_nbest_host())
    lib.ctcnbest_host_expand.argtypes = [_i32p, _i32p, _u32p, ctypes.c_longlong] + [ctypes.c_int] * 5 + [_i32p, _i32p, _u8p, _i32p]
    lib.ctcnbest_host_expand_full.argtypes = [_i32p, _i32p, _u32p] + [ctypes.c_int] * 3 + [_i32p, _i32p]
    lib.ctcnbest_host_lds_bytes.restype = ctypes.c_longlong
    lib.ctcnbest_host_vec16.argtypes = [ctypes.c_int, ctypes.c_ulonglong, ctypes.c_ulonglong]
    return lib


def _records(hdr, ent, lab):
    hdr, ent = np.ascontiguousarray(hdr, np.int32), np.ascontiguousarray(ent, np.int32)
    n_labels = int(np.asarray(lab).size)
    buf = np.ascontiguousarray(lab, np.uint32) if n_labels else np.zeros((1,), np.uint32)  # (a non-null pointer; n_labels stays 0)
    return hdr, ent, buf, n_labels


def host_nbest(hdr, ent, lab, T, n, method=0, fill=0x5A5A5A5A):
    """The twin's n-best expansion over buffers of ``fill`` words: method 0 = the product's host expansion (one row buffer), 1 = the
    kernel's segment walk.  -> (tokens [B,n,T], timesteps [B,n,T], row_ok bool [B,n], status [B])."""
    hdr, ent, buf, n_labels = _records(hdr, ent, lab)
    B, K = ent.shape[:2]
    tok = np.full((B, n, T), fill, np.int32)
    ts = np.full((B, n, T), fill, np.int32)
    ok = np.full((B, n), 9, np.uint8)
    st = np.full((B,), -1, np.int32)
    rc = _lib().ctcnbest_host_expand(hdr.ctypes.data_as(_i32p), ent.ctypes.data_as(_i32p), buf.ctypes.data_as(_u32p), n_labels, B, K, T, n, method,
                                     tok.ctypes.data_as(_i32p), ts.ctypes.data_as(_i32p), ok.ctypes.data_as(_u8p), st.ctypes.data_as(_i32p))
    assert rc >= 0, "the twin refused its arguments"
    assert rc == int((st != 0).sum())
    return tok, ts, ok.astype(bool), st


def host_full(hdr, ent, lab, T):
    """The full host expansion (compact_results.h expand_item_host) -> (tokens [B,K,T], timesteps [B,K,T])."""
    hdr, ent, buf, _ = _records(hdr, ent, lab)
    B, K = ent.shape[:2]
    tok = np.full((B, K, T), 0x5A5A5A5A, np.int32)
    ts = np.full((B, K, T), 0x5A5A5A5A, np.int32)
    rc = _lib().ctcnbest_host_expand_full(hdr.ctypes.data_as(_i32p), ent.ctypes.data_as(_i32p), buf.ctypes.data_as(_u32p), B, K, T,
                                          tok.ctypes.data_as(_i32p), ts.ctypes.data_as(_i32p))
    assert rc == 0
    return tok, ts


def host_threads(n):
    return int(_lib().ctcnbest_host_threads(int(n)))


def host_lds_bytes(K, n):
    return int(_lib().ctcnbest_host_lds_bytes(int(K), int(n)))


def host_vec16(T, tok_addr=0, ts_addr=0):
    return bool(_lib().ctcnbest_host_vec16(int(T), int(tok_addr), int(ts_addr)))


# ---- inputs the GPU tests share ------------------------------------------------------------------------------------------------------
_CACHE = {}


def cached(key, make):
    """A reference computed once, shared among the tests that need it, and left unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]
