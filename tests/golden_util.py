"""Loader for the committed reference fixtures (tests/golden/*.npz, made by tests/golden/make_golden.py)."""
import glob
import hashlib
import os

import numpy as np

import oracle_util as ou

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    beam, top_n, blank, log_input = (int(v) for v in z["params"])
    seq_lens = z["seq_lens"] if z["seq_lens"].size else None
    args = dict(probs=z["probs"], seq_lens=seq_lens, beam=beam, cutoff_top_n=top_n, blank_id=blank,
                log_input=bool(log_input), cutoff_prob=float(z["cutoff_prob"]))
    want = dict(tokens=z["tokens"], timesteps=z["timesteps"], scores=z["scores"], lens=z["lens"], nres=z["nres"])
    return args, want


GOLDEN_LM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_lm")
DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def lm_names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_LM_DIR, "*.npz")))


def load_lm(name):
    """LM-tier fixtures (tests/golden/make_golden_lm.py): decode arguments, scorer arguments, the reference's outputs."""
    z = np.load(os.path.join(GOLDEN_LM_DIR, name + ".npz"))
    beam, top_n, blank, log_input = (int(v) for v in z["params"])
    seq_lens = z["seq_lens"] if z["seq_lens"].size else None
    args = dict(probs=z["probs"], seq_lens=seq_lens, beam=beam, cutoff_top_n=top_n, blank_id=blank, log_input=bool(log_input))
    lm = dict(alpha=float(z["alpha_beta"][0]), beta=float(z["alpha_beta"][1]), lm_path=os.path.join(DATA_DIR, str(z["arpa"])),
              labels=[str(x) for x in z["labels"]], meta=tuple(int(v) for v in z["meta"]))
    want = dict(tokens=z["tokens"], timesteps=z["timesteps"], scores=z["scores"], lens=z["lens"], nres=z["nres"])
    return args, lm, want


# The reference's results for the inputs of the live differential tests (tests/golden/make_golden_live.py): where oracle/_ref
# is not built those tests compare against these instead of skipping.
LIVE_DIR = os.path.join(GOLDEN_DIR, "live")


def input_digest(x, **kw):
    """sha256 of one decode call's inputs: the array (as float32) with its shape, then the keyword arguments by name."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    h = hashlib.sha256(repr(x.shape).encode())
    h.update(x.tobytes())
    for k in sorted(kw):
        v = kw[k].tolist() if isinstance(kw[k], np.ndarray) else kw[k]
        h.update(("%s=%r;" % (k, v)).encode())
    return h.hexdigest()


def reference_result(name, x, **kw):
    """The reference's ``ou.decode(x, **kw)`` (no LM): run by oracle/_ref where it is built -- and then also checked against
    the stored copy -- else read from tests/golden/live/<name>.npz, which must have been made from the same inputs."""
    path = os.path.join(LIVE_DIR, name + ".npz")
    stored = None
    if os.path.exists(path):
        z = np.load(path)
        assert str(z["input_sha256"]) == input_digest(x, **kw), "%s: the stored reference result belongs to other inputs" % name
        stored = {k: z[k] for k in ("tokens", "timesteps", "scores", "lens", "nres")}
    if not ou.have_reference():
        assert stored is not None, "%s: oracle/_ref is not built and there is no stored result %s" % (name, path)
        return stored
    live = ou.decode(x, which="reference", **kw)
    if stored is not None:
        ou.assert_same(live, stored, name + " (stored reference result vs live reference)")
    return live
