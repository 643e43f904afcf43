"""Helpers of the CTC prefix score tests (TEST INFRASTRUCTURE ONLY): the definitions of include/ctcdecode_amd.h "CTC prefix scores"
restated in numpy from the header's text and not from prefix.h (sequential in t, vectorised over the candidates, the box's expf / logf,
loglik_util's lse3), loglik_util.forward's recurrence with its last two columns kept, and the case builder.  The blank is label 0."""
import align_util as au
import loglik_util as lu
import numpy as np

F32, NEG_INF = np.float32, np.float32(-np.inf)
_vexpf, _vlogf = np.vectorize(lu.expf, otypes=[np.float32]), np.vectorize(lu.logf, otypes=[np.float32])


# ---- one prefix of one item.  lp float32 [T, V]; n frames of it count; cols float32 [T, 2] = (r_n, r_b), NaN from n on ---------------
def r_init(lp, n):
    cols = np.full((lp.shape[0], 2), np.nan, np.float32)
    for t in range(n):
        cols[t] = NEG_INF, (F32(lp[0, 0]) if t == 0 else F32(F32(lp[t, 0]) + lu.lse3(cols[t - 1, 1], NEG_INF, NEG_INF)))
    return cols


def r_advance(lp, n, pcols, L, last, c):
    cols = np.full((lp.shape[0], 2), np.nan, np.float32)
    with np.errstate(all="ignore"):
        for t in range(n):
            if t == 0:
                cols[0] = (F32(lp[0, c]) if L == 0 else NEG_INF), NEG_INF
                continue
            skip = pcols[t - 1, 0] if (L == 0 or c != last) else NEG_INF
            cols[t] = (F32(F32(lp[t, c]) + lu.lse3(cols[t - 1, 0], pcols[t - 1, 1], skip)), F32(F32(lp[t, 0]) + lu.lse3(cols[t - 1, 1], cols[t - 1, 0], NEG_INF)))
    return cols


def r_eos(n, cols, L):
    return lu.lse3(cols[n - 1, 1], cols[n - 1, 0] if L >= 1 else NEG_INF, NEG_INF) if n else (F32(0.0) if L == 0 else NEG_INF)


def r_scores(lp, n, cols, L, last, cands):
    """psi of the valid candidates ``cands`` (int array) -> float32 array: the (m, s) pass, every step one float32 operation."""
    m, s = np.full(len(cands), NEG_INF, np.float32), np.zeros(len(cands), np.float32)
    with np.errstate(all="ignore"):
        for t in range(n):
            if t == 0:
                v = lp[0, cands].astype(np.float32) if L == 0 else np.full(len(cands), NEG_INF, np.float32)
            else:
                rn, rb = cols[t - 1]
                v = lp[t, cands].astype(np.float32) + np.where((cands == last) & (L >= 1), rb, lu.lse3(rb, rn, NEG_INF)).astype(np.float32)
            take = v > NEG_INF
            up = take & (v > m)
            s_up = (s * _vexpf(np.where(up, m - v, F32(0.0)).astype(np.float32))).astype(np.float32) + F32(1.0)
            s_dn = s + _vexpf(np.where(take & ~up, v - m, F32(0.0)).astype(np.float32))
            s, m = np.where(up, s_up, np.where(take, s_dn, s)).astype(np.float32), np.where(up, v, m).astype(np.float32)
        return np.where(m > NEG_INF, _vlogf(np.where(m > NEG_INF, s, F32(1.0))) + m, NEG_INF).astype(np.float32)


def lattice_cols(lp, n, y):
    """loglik_util.forward's loop over a[t][s] for the labels ``y``, with a[t][S-2] and a[t][S-1] of every frame kept -> [T, 2]."""
    S = 2 * len(y) + 1
    z = [0 if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    cols, a = np.full((lp.shape[0], 2), np.nan, np.float32), [F32(lp[0, z[s]]) if s < 2 else NEG_INF for s in range(S)]
    with np.errstate(all="ignore"):
        for t in range(n):
            if t:
                a = [F32(F32(lp[t, z[s]]) + lu.lse3(a[s], a[s - 1] if s else NEG_INF, a[s - 2] if s >= 3 and s % 2 and z[s] != z[s - 2] else NEG_INF)) for s in range(S)]
            cols[t] = (a[S - 2] if S >= 2 else NEG_INF), a[S - 1]
    return cols


# ---- the slots of a batch.  A state: dict(cols [B, R, T, 2], last [B, R], lens [B, R]); c: a case of make_case ------------------------
def state(c, R):
    B, T, _ = c["lp"].shape
    return dict(cols=np.full((B, R, T, 2), np.nan, np.float32), last=np.full((B, R), -1, np.int32), lens=np.full((B, R), -1, np.int32))


def init(c, R):
    st = state(c, R)
    for b, n in enumerate(c["seq_lens"]):
        st["cols"][b, 0], st["lens"][b, 0] = r_init(c["lp"][b], n), 0
    return st


def scores(c, st, cands=None):
    """-> (scores [B, R, C], eos [B, R]); ``cands`` [B, R, C] or None: all labels.  -inf for unused slots and candidates outside [1, V)."""
    V = c["lp"].shape[2]
    cands = np.broadcast_to(np.arange(V, dtype=np.int32), st["lens"].shape + (V,)) if cands is None else cands
    out, eos = np.full(cands.shape, NEG_INF, np.float32), np.full(st["lens"].shape, NEG_INF, np.float32)
    for b, r in np.argwhere(st["lens"] >= 0):
        lp, n, cols, L, k = c["lp"][b], c["seq_lens"][b], st["cols"][b, r], st["lens"][b, r], cands[b, r]
        eos[b, r] = r_eos(n, cols, L)
        out[b, r, (k > 0) & (k < V)] = r_scores(lp, n, cols, L, st["last"][b, r], k[(k > 0) & (k < V)])
    return out, eos


def advance(c, st, parents, labels):
    new = state(c, parents.shape[1])
    for b, j in np.argwhere(parents >= 0):
        p = parents[b, j]
        new["cols"][b, j] = r_advance(c["lp"][b], c["seq_lens"][b], st["cols"][b, p], st["lens"][b, p], st["last"][b, p], labels[b, j])
        new["last"][b, j], new["lens"][b, j] = labels[b, j], st["lens"][b, p] + 1
    return new


def same_bits(got, want, what, c=None):
    """Bit for bit as uint32; with the case ``c``: cols [B, R, T, 2], compared below each item's n and where ``want`` is defined."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    keep = np.ones(got.shape, bool) if c is None else (np.arange(got.shape[2])[None, None, :, None] < c["seq_lens"][:, None, None, None]) & ~np.isnan(want)
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & keep)
    assert bad.size == 0, "%s: differs at %s: got %r, want %r" % (what, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def make_case(T, V, seq_lens, R, seed, C=5, inf_frames=()):
    """Log-softmax rows [B, T, V] with 3 % of the entries -inf, label 1 -inf throughout item 0, and the frames ``inf_frames`` -inf in
    every label.  Three steps for R slots: parents (step 0: the empty prefix, slot R - 1 left unused; then slots reordered and
    repeated), labels (slot 1 repeats its parent's last) and lists [B, R, C] with -1, the blank and the slot's last label among them."""
    rng = np.random.default_rng(seed)
    B = len(seq_lens)
    lp = au.log_softmax_rows(rng, B, T, V)
    lp[rng.random(lp.shape) < 0.03] = NEG_INF
    lp[0, :, 1] = NEG_INF
    lp[:, list(inf_frames)] = NEG_INF
    labels = [rng.integers(1, V, (B, R)).astype(np.int32) for _ in range(3)]
    parents = [np.zeros((B, R), np.int32), rng.integers(0, max(R - 1, 1), (B, R)).astype(np.int32), rng.integers(0, R, (B, R)).astype(np.int32)]
    cands = [rng.integers(0, V, (B, R, C)).astype(np.int32) for _ in range(3)]
    if R > 1:
        parents[0][:, R - 1] = -1
    for k in (1, 2):
        labels[k][:, 1 % R] = np.take_along_axis(labels[k - 1], parents[k][:, 1 % R, None], 1)[:, 0]
        cands[k][:, :, 0], cands[k][:, :, 1], cands[k][:, :, 2] = labels[k - 1], -1, 0
    texts = {(b, 0): [] for b in range(B)}  # the labels of every slot after the three steps
    for k in range(3):
        texts = {(b, j): texts[(b, p)] + [labels[k][b, j]] for b in range(B) for j, p in enumerate(parents[k][b]) if p >= 0}
    return dict(lp=lp, seq_lens=np.asarray(seq_lens, np.int32), R=R, parents=parents, labels=labels, cands=cands, texts=texts)
