"""Helpers of the stream-image tests (TEST INFRASTRUCTURE ONLY): the host twin (tests/native/snapshot_host.cpp: the stream of
commit_util.HostStream with ctcdecode_amd/csrc/stream_snapshot.h's save / check / restore run on its parked state), the image's size
restated from the format's description, and the words of an image by name -- for the tests that corrupt one."""
import ctypes
import os

import commit_util as mu
import numpy as np
import oracle_util as ou

ROOT = ou.ROOT
SNAPSHOT_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcsnapshot_host.so")
NATIVE = os.path.join(ROOT, "tests", "native")
GOLDEN = os.path.join(ROOT, "tests", "golden")

_u8p = ctypes.POINTER(ctypes.c_ubyte)

# the format, restated (include/ctcdecode_amd.h): 16 header words, 12 state words, A * K array words, 5 M node words
HDR_WORDS, STATE_WORDS, ARRAYS_PLAIN, ARRAYS_LM = 16, 12, 14, 26
MAGIC = 0x53435443
W_MAGIC, W_VERSION, W_TOTAL, W_BEAM, W_LABELS, W_KIND, W_FP, W_FRAMES, W_COMMITTED, W_NODES, W_ARRAYS = 0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 13
S_FRAMES, S_N, S_POOL, S_WLOG = 0, 1, 2, 3
A_NODE, A_PAR, A_CH, A_DEP, A_LCP, A_VIA, A_VIAANC, A_VIACH, A_UP, A_FIN = 0, 1, 2, 3, 4, 5, 6, 7, 8, 13
A_LMST, A_DN, A_DFC, A_SPST = 14, 18, 21, 24


def image_bytes(K, lm, M):
    return 4 * (HDR_WORDS + STATE_WORDS + (ARRAYS_LM if lm else ARRAYS_PLAIN) * K + 5 * M)


def words(blob):
    """A writable int32 copy of the image's words."""
    return np.frombuffer(bytes(blob), dtype="<i4").copy()


def array_word(K, a, j):
    return HDR_WORDS + STATE_WORDS + a * K + j


def node_word(K, lm, M, i, part=0):
    """part 0: the node's parent word; 1: its express word; 2: the high part of its time step."""
    base = HDR_WORDS + STATE_WORDS + (ARRAYS_LM if lm else ARRAYS_PLAIN) * K
    return base + (3 * i if part == 0 else 3 * M + i if part == 1 else 4 * M + i)


def build_snapshot_host():
    import subprocess

    src = os.path.join(NATIVE, "snapshot_host.cpp")
    csrc = os.path.join(ROOT, "ctcdecode_amd", "csrc")
    deps = [src] + [os.path.join(NATIVE, f) for f in ("commit_host.cpp", "compact_host.cpp", "peek_host.cpp", "core_host.cpp")] + \
        [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if os.path.exists(SNAPSHOT_HOST_SO) and all(os.path.getmtime(SNAPSHOT_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return SNAPSHOT_HOST_SO
    os.makedirs(os.path.dirname(SNAPSHOT_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (SNAPSHOT_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-DCTC_ASSUME_CHECKED", src, "-o", tmp, "-lpthread"], check=True)
    os.replace(tmp, SNAPSHOT_HOST_SO)
    return SNAPSHOT_HOST_SO


class Refused(ValueError):
    """An image the check turned away: ``code`` (SNAP_*), ``name``, ``at``."""

    def __init__(self, code, name, at):
        ValueError.__init__(self, "image refused: %s (code %d, at %d)" % (name, code, at))
        self.code, self.name, self.at = code, name, at


class HostStream(mu.HostStream):
    """One stream of the host twin: commit_util.HostStream's feed(), peek(), compact() and commit(), and save() / restore()."""

    def __init__(self, V, beam, frames_hint, **kw):
        saved = mu.build_commit_host
        mu.build_commit_host = build_snapshot_host  # (the twin's library holds the other twins as they are)
        try:
            mu.HostStream.__init__(self, V, beam, frames_hint, **kw)
        finally:
            mu.build_commit_host = saved
        self.config = (V, beam, dict(kw))
        lib = self.lib
        lib.ctcsnap_host_save.argtypes = [ctypes.c_void_p, ctypes.c_longlong, _u8p, ctypes.c_longlong]
        lib.ctcsnap_host_save.restype = ctypes.c_longlong
        lib.ctcsnap_host_check.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
        lib.ctcsnap_host_restore.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
        lib.ctcsnap_host_info.argtypes = [ctypes.c_char_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_ulonglong)]
        lib.ctcsnap_host_fingerprint.argtypes = [ctypes.c_void_p]
        lib.ctcsnap_host_fingerprint.restype = ctypes.c_ulonglong
        lib.ctcsnap_host_error_name.argtypes = [ctypes.c_int]
        lib.ctcsnap_host_error_name.restype = ctypes.c_char_p

    fingerprint = property(lambda self: int(self.lib.ctcsnap_host_fingerprint(self.c)))

    def save(self):
        """-> the stream's image (bytes).  Compacts the stream, as the product's save does."""
        n = self.lib.ctcsnap_host_save(self.c, self.committed_len, None, 0)
        if n < 0:
            raise RuntimeError("host stream: save returned %d" % n)
        buf = np.full((n + 16,), 0xA5, np.uint8)
        m = self.lib.ctcsnap_host_save(self.c, self.committed_len, ou._ptr(buf, _u8p), n)
        if m != n:
            raise RuntimeError("host stream: save returned %d, then %d" % (n, m))
        assert (buf[n:] == 0xA5).all(), "save wrote behind its image"
        return buf[:n].tobytes()

    def check(self, blob):
        """-> (code, name, at) of the check of `blob` against this stream's configuration (code 0: it would be accepted)."""
        blob = bytes(blob)
        at = ctypes.c_longlong(-1)
        code = self.lib.ctcsnap_host_check(self.c, blob, len(blob), ctypes.byref(at))
        return code, self.lib.ctcsnap_host_error_name(code).decode(), int(at.value)

    def restore(self, blob, frames_hint=0, committed=None, **other):
        """-> a NEW stream of this one's configuration (other: creation arguments that differ) holding the image.  committed: the
        (tokens, timesteps) the saved stream had committed -- the caller keeps them, as with the product."""
        blob = bytes(blob)
        V, beam, kw = self.config
        kw = dict(kw, **other)
        new = HostStream(kw.pop("V", V), kw.pop("beam", beam), 1, **kw)
        done = ctypes.c_longlong(-1)
        rc = self.lib.ctcsnap_host_restore(new.c, blob, len(blob), frames_hint, ctypes.byref(done))
        if rc > 0:
            raise Refused(rc, self.lib.ctcsnap_host_error_name(rc).decode(), new.check(blob)[2])
        if rc != 0:
            raise RuntimeError("host stream: restore returned %d" % rc)
        new.frames = info(blob)["frames"]
        tok, ts = committed if committed is not None else (np.zeros((0,), np.int32), np.zeros((0,), np.int32))
        assert len(tok) == int(done.value), "the image says %d labels were committed, the caller holds %d" % (done.value, len(tok))
        new.tokens, new.timesteps = np.array(tok, np.int32), np.array(ts, np.int32)
        return new


def info(blob):
    """The twin's snapshot_info as a dict, or Refused."""
    lib = ctypes.CDLL(build_snapshot_host())
    lib.ctcsnap_host_info.argtypes = [ctypes.c_char_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_ulonglong)]
    lib.ctcsnap_host_error_name.restype = ctypes.c_char_p
    blob = bytes(blob)
    out = (ctypes.c_ulonglong * 10)()
    rc = lib.ctcsnap_host_info(blob, len(blob), out)
    if rc != 0:
        raise Refused(rc, lib.ctcsnap_host_error_name(rc).decode(), -1)
    names = ("version", "beam", "labels", "scorer_kind", "nodes", "arrays", "frames", "committed", "fingerprint", "bytes")
    return dict((k, int(v)) for k, v in zip(names, out))


def one(res, b):
    """Item b of a result dict as a one-item result dict."""
    return dict((k, v[b:b + 1]) for k, v in res.items())
