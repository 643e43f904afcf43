"""-m gpu tests of the CTC prefix scores (``CTCBeamDecoder.prefix_init`` / ``prefix_scores`` / ``prefix_advance``): device output == the
numpy restatement of the header's definitions (tests/prefix_util.py), bit for bit as uint32, at the shapes where the kernels can go
wrong.  A case is a chain: init, then three times scores of all labels, scores of listed candidates, advance."""
import align_util as au
import numpy as np
import prefix_util as pu
import pytest

pytestmark = pytest.mark.gpu


def _dec(V, **kw):
    import ctcdecode_amd

    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=0, beam_width=8, **dict(dict(log_probs_input=True), **kw))


def _chain(dec, x, c, what):
    """The case's chain on the device, every output against the restatement.  -> the last state, its restated twin, the scores calls' kernels."""
    import torch

    seq, codes = torch.from_numpy(c["seq_lens"]), []
    st, ref = dec.prefix_init(x, seq, c["R"]), pu.init(c, c["R"])
    for k in range(4):
        pu.same_bits(st.cols.cpu().numpy(), ref["cols"], "%s: cols before step %d" % (what, k), c)
        assert np.array_equal(st.last.cpu().numpy(), ref["last"]) and np.array_equal(st.lens.cpu().numpy(), ref["lens"]), (what, k)
        if k == 3:
            return st, ref, codes
        for cands in (None, c["cands"][k]):
            sc, eos = dec.prefix_scores(x, seq, st, None if cands is None else torch.from_numpy(cands))
            codes.append(dec.last_prefix_kernel())
            wsc, weos = pu.scores(c, ref, cands)
            pu.same_bits(sc.cpu().numpy(), wsc, "%s: step %d: scores, listed %s" % (what, k, cands is not None))
            pu.same_bits(eos.cpu().numpy(), weos, "%s: step %d: eos" % (what, k))
        st = dec.prefix_advance(x, seq, st, torch.from_numpy(c["parents"][k]), torch.from_numpy(c["labels"][k]))
        ref = pu.advance(c, ref, c["parents"][k], c["labels"][k])


# n: 0, 1, 2 and both sides of the advance tile (16) and of the scores chunk (32); whole frames of -inf, one at the chunk's edge, on the
# staged route (V <= 128) and the gathered one.  C (listed) on both sides of a wave (64 / 65) and of the candidate tile (256 / 257); all
# labels beyond a tile (V 300).  R at H - 1, H, H + 1 (H = 8: V > 128, one lane group) and spread over eight lane groups (V 29, R 10).
# -> (the case, what the all-labels call reports: log2 of the lane group, prefixes per group)
CASES = {
    "frames": (dict(T=33, V=6, seq_lens=[33, 0, 1, 2, 15, 16, 17, 31, 32], R=4, seed=3), 5, 1),
    "inf_frames_staged": (dict(T=40, V=6, seq_lens=[40, 33, 32], R=4, seed=15, inf_frames=[5, 31]), 5, 1),
    "inf_frames_gathered": (dict(T=40, V=130, seq_lens=[40, 33], R=3, seed=16, inf_frames=[6, 32]), 8, 3),
    "north_star_groups": (dict(T=35, V=29, seq_lens=[35, 20], R=10, seed=4, C=40), 5, 2),
    "wave": (dict(T=9, V=64, seq_lens=[9, 5], R=3, seed=7, C=64), 6, 1),
    "wave_plus": (dict(T=9, V=65, seq_lens=[9, 5], R=3, seed=8, C=65), 7, 2),
    "tile": (dict(T=9, V=129, seq_lens=[9, 9], R=2, seed=10, C=256), 8, 2),
    "tile_plus": (dict(T=33, V=300, seq_lens=[33, 8], R=2, seed=11, C=257), 8, 2),
    "R7": (dict(T=9, V=130, seq_lens=[9, 3], R=7, seed=12), 8, 7),
    "R8": (dict(T=9, V=130, seq_lens=[9, 3], R=8, seed=13), 8, 8),
    "R9": (dict(T=9, V=130, seq_lens=[9, 3], R=9, seed=14), 8, 8),
}


@pytest.mark.parametrize("name", list(CASES))
def test_chain_equals_the_restatement(name):
    """Every step's scores, eos and cols[..., :n, :]: the empty prefix, candidates equal to the last label, -1 and blank, unused slots,
    repeated parents, prefixes longer than n.  The last state's eos == the device log_likelihood; (frames) its cols == the lattice's."""
    import torch

    (_, lg, hs), c = CASES[name], pu.make_case(**CASES[name][0])
    dec, x = _dec(c["lp"].shape[2]), torch.from_numpy(c["lp"]).cuda()
    st, ref, codes = _chain(dec, x, c, name)
    assert (codes[0] >> 5 & 3, codes[0] >> 8 & 15, codes[0] >> 12) == (0, lg, hs), hex(codes[0])
    (B, R), texts, seq = ref["lens"].shape, c["texts"], torch.from_numpy(c["seq_lens"])
    tok = torch.tensor([[texts[(b, j)] for j in range(R)] for b in range(B)], dtype=torch.int32).cuda()
    ll = dec.log_likelihood(x, seq, tok, torch.full((B, R), 3, dtype=torch.int32).cuda()).cpu().numpy()
    pu.same_bits(dec.prefix_scores(x, seq, st)[1].cpu().numpy(), ll, name + ": eos against log_likelihood")
    if name == "frames":
        want = np.asarray([[pu.lattice_cols(c["lp"][b], c["seq_lens"][b], texts[(b, j)]) for j in range(R)] for b in range(B)])
        pu.same_bits(st.cols.cpu().numpy(), want, "cols against the lattice", c)


@pytest.mark.parametrize("V", [128, 129])
@pytest.mark.parametrize("mode", ["log", "prob"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_every_instantiation(dtype, mode, V):
    """3 dtypes x 2 input modes x staged (V 128) / gathered (V 129), and in each chain all labels / listed: the 24 scores kernels and
    the 12 advance / init kernels, each against the restatement on the rows' float32 copies; ctcd_last_prefix_kernel names them."""
    import torch

    c = pu.make_case(T=5, V=V, seq_lens=[5, 4], R=2, seed=20)
    x = torch.from_numpy(c["lp"]).cuda()
    x = (x.exp() if mode == "prob" else x).to(dict(f32=torch.float32, f16=torch.float16, bf16=torch.bfloat16)[dtype])
    wide, dec = x.float().cpu().numpy(), _dec(V, log_probs_input=mode == "log")
    _, _, codes = _chain(dec, x, dict(c, lp=au.prob_to_lp(wide) if mode == "prob" else wide), "%s %s" % (dtype, mode))
    base = dict(f32=0, f16=1, bf16=2)[dtype] + (4 if mode == "prob" else 0) + (8 if V == 128 else 0)
    assert [k & 127 for k in codes] == [base, base + 16] * 3 and dec.last_prefix_kernel() & 127 == (base & 7) + 32, codes


def test_invalid_entries_raise_and_spare_the_other_items():
    """A candidate outside [-1, V): ValueError; with the caller's status tensor the item's word is raised instead, the entry scores
    -inf and every other result is the restatement's.  A label = V and a parent that is no live slot: the same, the child unused."""
    import torch

    c = pu.make_case(T=9, V=7, seq_lens=[9, 6, 9], R=3, seed=30)
    dec, x, seq = _dec(7), torch.from_numpy(c["lp"]).cuda(), torch.from_numpy(c["seq_lens"])
    st, ref = dec.prefix_advance(x, seq, dec.prefix_init(x, seq, 3), *map(torch.from_numpy, (c["parents"][0], c["labels"][0]))), pu.advance(c, pu.init(c, 3), c["parents"][0], c["labels"][0])
    cands = c["cands"][1].copy()
    cands[1, 0, 3], cands[1, 1, 4] = 7, -2
    with pytest.raises(ValueError, match="BAD_ROW"):
        dec.prefix_scores(x, seq, st, torch.from_numpy(cands))
    status = torch.zeros(3, dtype=torch.int32, device="cuda")
    sc, eos = dec.prefix_scores(x, seq, st, torch.from_numpy(cands), status=status)
    wsc = pu.scores(c, ref, cands)[0]
    assert status.tolist() == [0, 8, 0] and np.isneginf(wsc[1, 0, 3]) and np.isfinite(wsc[1, 0, 0])
    pu.same_bits(sc.cpu().numpy(), wsc, "scores beside an invalid candidate")
    for p, lab in ((1, 7), (2, 1), (3, 1)):  # (a label = V; slot 2 is unused; there is no slot 3)
        parents, labels = np.zeros((3, 3), np.int32), np.ones((3, 3), np.int32)
        parents[1, 1], labels[1, 1] = p, lab
        with pytest.raises(ValueError, match="BAD_ROW"):
            dec.prefix_advance(x, seq, st, torch.from_numpy(parents), torch.from_numpy(labels))
        new = dec.prefix_advance(x, seq, st, torch.from_numpy(parents), torch.from_numpy(labels), status=status.zero_())
        parents[1, 1] = -1  # (what the invalid child comes out as: unused)
        want = pu.advance(c, ref, parents, labels)
        assert status.tolist() == [0, 8, 0] and np.array_equal(new.lens.cpu().numpy(), want["lens"])
        pu.same_bits(new.cols.cpu().numpy(), want["cols"], "cols beside an invalid child", c)


def test_raw_logits_equal_the_call_on_log_softmax_rows():
    import torch

    c = pu.make_case(T=18, V=9, seq_lens=[18, 11], R=3, seed=40)
    logits = torch.from_numpy((np.random.default_rng(41).standard_normal(c["lp"].shape) * 3).astype(np.float32)).cuda()
    dec = _dec(9, log_probs_input=False, logits_input=True)
    _chain(dec, logits, dict(c, lp=dec.log_softmax(logits, torch.from_numpy(c["seq_lens"])).cpu().numpy()), "logits")
