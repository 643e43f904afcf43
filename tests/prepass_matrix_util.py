"""One case per pre-pass kernel instantiation of ctcdecode_amd/csrc/prepass.hip (the table ctcd_debug_prepass_table reports), plus
the global-memory route of prune_resolve_kernel for each input dtype: 89 cases.  Each names the instantiation it is for (``target``),
the decoder arguments and switches that select it, and an input recipe.  Shared by the CPU coverage check (test_abi.py: the targets
equal the build's table exactly) and the GPU tests (test_gpu_prepass_matrix.py).  No torch here: the CPU suite imports this module.

An instantiation is (kernel, a, b, dtype) as ``CTCBeamDecoder.last_prepass()`` names it: kernel "prob_to_log" / "widen" / "lsm_wave" /
"lsm_wg" (a = F4) / "prune_rows" (a = R) / "prune_wg" (a = F4, b = REG) / "prune_logits" (a = F4) / "resolve" (b = 1: its arrays in
global memory); dtype "f32" / "f16" / "bf16".  ``expected_prepass`` restates the dispatch of decode_common: what each stage of a case
must launch."""
import numpy as np

DTYPES = ("f32", "f16", "bf16")
B, T = 4, 24
LDS_BYTES = 160 * 1024  # one workgroup's LDS on gfx950


def _case(target, V, li, dt, top_n=None, cp=1.0, K=6, fused=True, reg=True, resolve_global=False, misaligned=False, ties=False):
    assert dt in DTYPES and li in (0, 1, 2)
    return dict(target=target, V=V, li=li, dt=dt, top_n=V if top_n is None else top_n, cp=cp, K=K, fused=fused, reg=reg,
                resolve_global=resolve_global, misaligned=misaligned, ties=ties)


def _f4(V):
    return 1 if V <= 1024 else 2 if V <= 2048 else 4 if V <= 4096 else 10 if V <= 10240 else 16


def _r(V):
    return 1 if V <= 64 else 4 if V <= 256 else 16 if V <= 1024 else 64 if V <= 4096 else 160 if V <= 10240 else 0


def _cases():
    C = []
    # the shapes differ from one dtype to the next, so that together they sit on both sides of every boundary of the dispatch
    for i, dt in enumerate(DTYPES):
        # ---- elementwise (no vocabulary prune): probabilities -> log; half log-probability rows widened.  bf16: a negative cutoff_prob
        # means no cumulative cut (the reference: log(-0.5) is NaN), so with cutoff_top_n >= V nothing is pruned
        C.append(_case(("prob_to_log", 0, 0, dt), V=(29, 64, 65)[i], li=0, dt=dt, cp=(1.0, 1.5, -0.5)[i]))
        # ---- log_softmax, one wave per row: short rows, V not a multiple of 4, and (bf16) logits 2 bytes off their alignment in front
        # of what would otherwise be the fused prune
        C.append(_case(("lsm_wave", 0, 0, dt), V=(29, 257, 1028)[i], li=2, dt=dt, top_n=(29, 257, 40)[i], cp=(1.0, 1.0, 0.99)[i],
                       misaligned=dt == "bf16"))
        # ---- log_softmax, a workgroup per row: unpruned, or in front of a prune that keeps more than 64 (not the fused pass)
        for F4, V in zip((1, 2, 4, 10, 16), [(260, 1028, 2052, 4100, 10244), (1024, 2048, 4096, 10240, 16384), (1024, 1028, 2052, 4100, 16384)][i]):
            unpruned = V <= 1024
            C.append(_case(("lsm_wg", F4, 0, dt), V=V, li=2, dt=dt, top_n=V if unpruned else 65, cp=1.0 if unpruned or F4 == 4 else 0.6,
                           K=4 if unpruned else 6))
        # ---- prune_rows_kernel: short rows, V not a multiple of 4, more than 64 kept, rows misaligned for the workgroup kernel
        C.append(_case(("prune_rows", 1, 0, dt), V=64, li=(1, 0, 1)[i], dt=dt, top_n=(40, 100, 64)[i], cp=(0.99, 0.6, 0.3)[i]))
        C.append(_case(("prune_rows", 4, 0, dt), V=(65, 256, 130)[i], li=(0, 1, 1)[i], dt=dt, top_n=(64, 40, 1)[i], cp=(1.0, 0.3, 1.0)[i]))
        # (float32: 4 bytes, half: 2 bytes past an aligned base -- the workgroup kernels' 16- / 8-byte loads would be misaligned)
        C.append(_case(("prune_rows", 16, 0, dt), V=1024, li=(1, 1, 0)[i], dt=dt, top_n=40, cp=(1.0, 0.6, 0.99)[i], misaligned=True))
        C.append(_case(("prune_rows", 64, 0, dt), V=(1026, 2048, 4096)[i], li=1, dt=dt, top_n=(40, 65, 65)[i], cp=(0.99, float("nan"), 1.0)[i]))
        C.append(_case(("prune_rows", 160, 0, dt), V=(4100, 10239, 10240)[i], li=(1, 0, 1)[i], dt=dt, top_n=(65, 40, 80)[i], cp=(1.0, 0.99, 0.6)[i]))
        C.append(_case(("prune_rows", 0, 0, dt), V=(16388, 12001, 10244)[i], li=(1, 1, 0)[i], dt=dt, top_n=(40, 40, 65)[i], cp=(0.99, 1.0, 1.0)[i]))
        # ---- the workgroup prune, the row read twice (switch) -- and beyond 10240 labels, where that is the only form
        for F4, V in zip((1, 2, 4, 10, 16), [(260, 2048, 2052, 10240, 16384), (1024, 1028, 4096, 4100, 10244), (260, 2048, 4096, 10240, 16384)][i]):
            C.append(_case(("prune_wg", F4, 0, dt), V=V, li=0 if F4 == 2 else 1, dt=dt, top_n=64 if F4 in (2, 16) else 40,
                           cp=-0.5 if (F4, dt) == (4, "f32") else 0.6 if F4 == 10 else 0.99, reg=F4 == 16))
        # ---- the workgroup prune, the row in registers (the default)
        for F4, V in zip((1, 2, 4, 10), [(1024, 1028, 4096, 4100), (260, 2048, 2052, 10240), (1024, 1028, 4096, 4100)][i]):
            C.append(_case(("prune_wg", F4, 1, dt), V=V, li=1 if F4 != 4 else 0, dt=dt, top_n=(40, 64, 1, 40)[(F4 > 1) + (F4 > 2) + (F4 > 4)],
                           cp=0.3 if F4 == 1 else 1.0 if F4 == 4 else 0.99))
        # ---- raw logits -> candidates in one pass
        for F4, V in zip((1, 2, 4, 10, 16), [(1024, 2048, 2052, 10240, 16388 - 4), (260, 1028, 4096, 4100, 16384), (1024, 2048, 4096, 10240, 10244)][i]):
            C.append(_case(("prune_logits", F4, 0, dt), V=V, li=2, dt=dt, top_n=64 if F4 == 2 else 40, cp=0.6 if F4 in (1, 10) else 0.99))
        # ---- the replay of tie frames (std::sort + the exact cumulative chain), its arrays in LDS and in global memory
        C.append(_case(("resolve", 0, 0, dt), V=(1000, 2048, 260)[i], li=(1, 1, 0)[i], dt=dt, top_n=40, cp=(0.99, 1.0, 0.6)[i], ties=True))
        C.append(_case(("resolve", 0, 1, dt), V=(1000, 2048, 260)[i], li=(1, 0, 1)[i], dt=dt, top_n=40, cp=(1.0, 0.6, 0.99)[i], ties=True,
                       resolve_global=True))
        if dt != "f32":  # half log-probability rows widened in front of the decode
            C.append(_case(("widen", 0, 0, dt), V=(65, 29)[i - 1], li=1, dt=dt, cp=(1.0, 1.5)[i - 1]))
    return C


CASES = _cases()
for _i, _c in enumerate(CASES):
    _c["seed"] = 7300 + 13 * _i


def case_id(c):
    k, a, b, dt = c["target"]
    name = {"prune_wg": "prune_wg%d_reg%d" % (a, b), "resolve": "resolve_%s" % ("global" if b else "lds")}.get(k, k + (str(a) if k in ("lsm_wg", "prune_rows", "prune_logits") else ""))
    return "%s_%s" % (name, dt)


def cuts(cp):
    """The reference's test for its cumulative cut: log(cutoff_prob) < 0.0, i.e. 0 <= cutoff_prob < 1 (NaN and negatives: no cut)."""
    return bool(0.0 <= cp < 1.0)


def pruned(c):
    return cuts(c["cp"]) or c["top_n"] < c["V"]


def resolve_lds_bytes(V, n):
    """prepass.h prune_resolve_lds_bytes."""
    cap = V // 17 + 2
    return V * 8 + 2 * (V + 2) * 2 + 6 * cap * 2 + 2 * (V // 2 + 1) * 2 + 3 * 64 * 4 + 64 + n * 4 + 64


def expected_prepass(c):
    """What decode_common launches for case c, stage by stage (as last_prepass() reports it)."""
    V, li, dt, n = c["V"], c["li"], c["dt"], min(c["top_n"], c["V"])
    aligned = not c["misaligned"]
    wg_shape = V % 4 == 0 and 256 < V <= 16384
    out = dict(elementwise=None, log_softmax=None, prune=None, resolve=None)
    fuse = li == 2 and pruned(c) and c["fused"] and wg_shape and n <= 64 and aligned
    if li == 2 and not fuse:
        out["log_softmax"] = ("lsm_wg", _f4(V), 0, dt) if wg_shape and aligned and c["fused"] else ("lsm_wave", 0, 0, dt)
        li, dt, aligned = 1, "f32", True  # (the normalised rows: float32, in the decoder's workspace)
    if pruned(c):
        if fuse:
            out["prune"] = ("prune_logits", _f4(V), 0, dt)
        elif wg_shape and n <= 64 and aligned:
            out["prune"] = ("prune_wg", _f4(V), int(c["reg"] and V <= 10240), dt)
        else:
            out["prune"] = ("prune_rows", _r(V), 0, dt)
        glob = c["resolve_global"] or resolve_lds_bytes(V, n) + 1024 > LDS_BYTES
        out["resolve"] = ("resolve", 0, int(glob), dt)
    elif li == 0 or dt != "f32":
        out["elementwise"] = ("prob_to_log" if li == 0 else "widen", 0, 0, dt)
    return out


def round_to(x, dt):
    """float32 array -> the nearest values of dtype dt (round to nearest even), as float32: what x.to(dtype).float() gives."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dt == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    if dt == "bf16":
        u = x.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        y = r.astype(np.uint32).view(np.float32)
        return np.where(np.isnan(x), x, y).astype(np.float32)
    return x


def inputs(c):
    """-> (x [B, T, V] float32 in the case's domain -- probabilities (li 0), log-probabilities (1) or logits (2) -- every value
    exactly representable in the case's dtype, seq_lens [B] int32 (T, 1, 0, T - 5), and the NaN positions).

    Frame kinds by t % 8: random; coarse (multiples of 0.5 in the log domain: exact ties inside and across the cut); peaky (the
    cumulative cut stops after a few labels); the top probability p0 with log(1 + p0) next to cutoff_prob (the cut decided within
    rounding distance); every third label -inf (probabilities: 0, and values near FLT_MIN); all -inf (all 0); rows that are not
    normalised; random with one NaN (pruned log / probability cases that keep fewer than V: the library defines NaN below every
    number).  A tie case (``ties``) makes every other frame coarse."""
    V, li, dt = c["V"], c["li"], c["dt"]
    rng = np.random.default_rng(c["seed"])
    z = rng.standard_normal((B, T, V)).astype(np.float64) * 2.0
    nan_ok = li != 2 and pruned(c) and c["top_n"] < V
    nans = []
    for b in range(B):
        for t in range(T):
            kind = t % 8
            if c["ties"] and t % 2 == 1:
                kind = 1
            row = z[b, t]
            if kind == 1:
                row = np.round(row * 2) / 2
                if li == 2:
                    z[b, t] = row
                    continue
                row = row - np.log(np.exp(row - row.max()).sum()) - row.max()
                z[b, t] = np.round(row * 2) / 2  # (log-probabilities on a 0.5 grid: ties, and a sum near 1)
                continue
            if kind == 2:
                row[rng.integers(0, V)] += 9.0
            if kind == 3 and li != 2 and cuts(c["cp"]):
                p0 = np.expm1(c["cp"])
                rest = rng.random(V) * 1e-6 / V
                rest[rng.integers(0, V)] = p0
                z[b, t] = np.log(rest)
                continue
            if kind == 6:
                if li == 2:
                    z[b, t] = row * 1e-4 + 9.0  # (all logits within 1e-3)
                else:
                    z[b, t] = np.log(rng.random(V) * 3.0)  # (probabilities that sum to about 1.5 V)
                continue
            if li == 2:
                z[b, t] = row
            else:
                z[b, t] = row - np.log(np.exp(row - row.max()).sum()) - row.max()
            if kind == 4:
                z[b, t, ::3] = -np.inf
            elif kind == 5:
                z[b, t] = -np.inf
            elif kind == 7 and nan_ok:
                nans.append((b, t, int(rng.integers(0, V))))
    x = np.exp(z) if li == 0 else z
    if li == 0:
        fr = x[:, 4::8]
        fr[..., 1::7] = rng.random(fr[..., 1::7].shape) * 4 * np.finfo(np.float32).tiny  # (near FLT_MIN: 0 to 4 * 2^-126)
    x = round_to(x.astype(np.float32), dt)
    for b, t, v in nans:
        x[b, t, v] = np.nan
    sl = np.array([T, 1, 0, T - 5], np.int32)
    return x, sl, nans
