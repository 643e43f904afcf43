"""Helpers of the tests of the blank-frame filter of live streams (TEST INFRASTRUCTURE ONLY): the ctypes front-end of the host twin
(tests/native/stream_blank_skip_host.cpp) -- a "stream" as the triple the library keeps, fed chunk by chunk -- and the chunk cutting the
CPU and GPU tests share.  The definition itself is blank_skip_util's: a filtered stream returns what ``blank_skip_util.decode`` returns
for the concatenation of its chunks."""
import ctypes
import os
import subprocess

import numpy as np
import blank_skip_util as bu

ROOT = bu.ROOT
NATIVE = bu.NATIVE
SSKIP_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcsskip_host.so")
DTYPES = bu.DTYPES

_i32p = ctypes.POINTER(ctypes.c_int32)
_llp = ctypes.POINTER(ctypes.c_longlong)


def build_sskip_host():
    src = os.path.join(NATIVE, "stream_blank_skip_host.cpp")
    deps = [src, os.path.join(ROOT, "ctcdecode_amd", "csrc", "stream_blank_skip.h"), os.path.join(ROOT, "ctcdecode_amd", "csrc", "blank_skip.h")]
    if os.path.exists(SSKIP_HOST_SO) and all(os.path.getmtime(SSKIP_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return SSKIP_HOST_SO
    os.makedirs(os.path.dirname(SSKIP_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (SSKIP_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, SSKIP_HOST_SO)
    return SSKIP_HOST_SO


_LIB = []


def lib():
    if not _LIB:
        so = ctypes.CDLL(build_sskip_host())
        pp = ctypes.POINTER(ctypes.c_void_p)
        so.ctcsskip_host_chunk.argtypes = [ctypes.c_void_p, ctypes.c_int, _i32p] + [ctypes.c_int] * 4 + [ctypes.c_float, pp, _llp, _llp, _i32p, _i32p]
        so.ctcsskip_host_remap_rows.argtypes = [_i32p, pp, _i32p, _i32p, pp, _i32p, ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
        so.ctcsskip_host_remap_rows.restype = None
        so.ctcsskip_host_remap_compact.argtypes = [_i32p, _i32p, ctypes.POINTER(ctypes.c_uint32), pp, _i32p, ctypes.c_int, ctypes.c_int]
        so.ctcsskip_host_remap_compact.restype = None
        so.ctcsskip_host_map_grown_cap.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
        so.ctcsskip_host_map_grown_cap.restype = ctypes.c_longlong
        so.ctcsskip_host_compact_route_ok.argtypes = [ctypes.c_longlong, ctypes.c_int]
        _LIB.append(so)
    return _LIB[0]


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data if a is not None and a.size else None for a in arrays])


def cuts(total, size):
    """[0, total) cut into chunks of ``size`` frames (the last one shorter): a list of (start, stop)."""
    return [(a, min(a + size, total)) for a in range(0, total, size)] or [(0, 0)]


class HostStreams(object):
    """B streams of the twin: ``feed(bits, seq_lens)`` is one chunk call; ``maps()`` the maps' used parts."""

    def __init__(self, B, dtype, blank_id, c):
        self.B, self.dtype, self.blank_id, self.c = B, dtype, blank_id, float(c)
        self.frames = np.zeros((B,), np.int64)
        self.seen = np.zeros((B,), np.int64)
        self._maps = [np.zeros((0,), np.int32) for _ in range(B)]

    def feed(self, bits, seq_lens=None):
        """``bits`` [B, T, V] storage (float32 or uint16 patterns).  -> (kept [B, T] with -1 where nothing was written, n' [B])."""
        B, T, V = bits.shape
        assert B == self.B
        if T == 0:  # (a chunk without frames: the twin wants a buffer; one frame of lengths 0)
            bits, T, seq_lens = np.zeros((B, 1, V), bits.dtype), 1, np.zeros((B,), np.int32)
        sl = None if seq_lens is None else np.ascontiguousarray(seq_lens, np.int32)
        for b in range(B):  # exactly frames + T entries, the tail poisoned: a write beyond the chunk's kept frames shows
            grown = np.full((int(self.frames[b]) + T,), -7, np.int32)
            grown[:int(self.frames[b])] = self._maps[b][:int(self.frames[b])]
            self._maps[b] = grown
        kept = np.full((B, T), -1, np.int32)
        n2 = np.full((B,), -1, np.int32)
        bits = np.ascontiguousarray(bits)
        rc = lib().ctcsskip_host_chunk(bits.ctypes.data, DTYPES[self.dtype], None if sl is None else sl.ctypes.data_as(_i32p), B, T, V, int(self.blank_id), self.c,
                                       _ptrs(self._maps), self.frames.ctypes.data_as(_llp), self.seen.ctypes.data_as(_llp), kept.ctypes.data_as(_i32p),
                                       n2.ctypes.data_as(_i32p))
        assert rc == 0, "the twin refused its arguments"
        for b in range(B):
            assert (self._maps[b][int(self.frames[b]):] == -7).all(), "the map was written beyond the kept frames"
        return kept, n2

    def maps(self):
        return [self._maps[b][:int(self.frames[b])].copy() for b in range(self.B)]


def host_remap_rows(ts, lens, maps, frames, since=None, rows=None):
    """The twin's row remap on a copy of ``ts`` [B, R, stride] (``rows``: per-item arrays remapped in place instead)."""
    B = len(maps)
    out = None if ts is None else np.ascontiguousarray(ts, np.int32).copy()
    R = 1 if out is None else out.shape[1]
    stride = max(len(r) for r in rows) if rows is not None else out.shape[2]
    ln = np.ascontiguousarray(lens, np.int32).reshape(-1)
    fr = np.ascontiguousarray(frames, np.int32)
    sn = None if since is None else np.ascontiguousarray(since, np.int32)
    maps = [np.ascontiguousarray(m, np.int32) for m in maps]
    lib().ctcsskip_host_remap_rows(None if out is None else out.ctypes.data_as(_i32p), None if rows is None else _ptrs(rows), ln.ctypes.data_as(_i32p),
                                   None if sn is None else sn.ctypes.data_as(_i32p), _ptrs(maps), fr.ctypes.data_as(_i32p), B, R, stride)
    return out


def host_remap_compact(hdr, ent, labels, maps, frames):
    lab = np.ascontiguousarray(labels, np.uint32).copy()
    if lab.size == 0:
        return lab
    B, K = ent.shape[:2]
    maps = [np.ascontiguousarray(m, np.int32) for m in maps]
    fr = np.ascontiguousarray(frames, np.int32)
    lib().ctcsskip_host_remap_compact(hdr.ctypes.data_as(_i32p), ent.ctypes.data_as(_i32p), lab.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _ptrs(maps),
                                      fr.ctypes.data_as(_i32p), B, K)
    return lab
