"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol include/ctcdecode_amd.h
declares (no compute calls -- there is no GPU here), and the Python class mirrors the reference's signature."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "ctcdecode_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ctcd_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g

    g.build()
    import ctypes

    from ctcdecode_amd import _build

    lib = ctypes.CDLL(_build.LIB_PATH)
    names = _declared()
    assert "ctcd_beam_decode" in names and "ctcd_beam_decode_host" in names and len(names) >= 9
    # the hook the GPU tests prove with which workspace layout (which kernel) a decode ran
    assert "ctcd_debug_last_layout" in names and "ctcd_debug_last_kernel" in names
    assert "ctcd_debug_last_prepass" in names and "ctcd_debug_prepass_table" in names
    from ctcdecode_amd import _native

    assert set(names) <= set(_native.SYMBOLS), sorted(set(names) - set(_native.SYMBOLS))
    for name in names:
        assert hasattr(lib, name), name
    lib.ctcd_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.ctcd_version()
    lib.ctcd_workgroup_lds_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double]
    assert 0 < lib.ctcd_workgroup_lds_bytes(100, 29, 40, 1.0) <= 160 * 1024  # BASELINE.json configs[1] fits one CU's LDS


def test_kernel_matrix_covers_every_instantiation():
    """tests/test_gpu_kernel_matrix.py has one case per instantiation the product build compiles (decode_kernel.h CTC_KERNEL_LIST,
    its #else branch): an instantiation added without a case, or a case whose kernel no longer exists, fails here."""
    import kernel_matrix_util as km

    listed = km.parse_kernel_list(open(os.path.join(ROOT, "ctcdecode_amd", "csrc", "decode_kernel.h")).read())
    assert len(listed) == 60 and len(set(listed)) == len(listed), len(listed)
    cases = [c["kernel"] for c in km.CASES]
    assert len(set(cases)) == len(cases), "two matrix cases expect the same kernel"
    assert set(cases) == set(listed), (sorted(set(listed) - set(cases)), sorted(set(cases) - set(listed)))
    assert len({km.case_id(c) for c in km.CASES}) == len(cases)


def test_prepass_matrix_covers_every_instantiation():
    """tests/test_gpu_prepass_matrix.py has one case per pre-pass instantiation the build compiles (the table the dispatch picks from,
    ctcd_debug_prepass_table) and one for the global-memory route of prune_resolve_kernel per dtype: an instantiation added without a
    case, or a case whose kernel no longer exists, fails here.  Each case's target is among the kernels the dispatch prescribes for it."""
    import __graft_entry__ as g

    g.build()
    import ctcdecode_amd
    import prepass_matrix_util as pm

    table = ctcdecode_amd.prepass_table()
    listed = [t[:4] for t in table]
    assert len(listed) == 86 and len(set(listed)) == len(listed), len(listed)
    counts = {}
    for k, a, b, dt in listed:
        counts[k] = counts.get(k, 0) + 1
    assert counts == dict(prob_to_log=3, widen=2, lsm_wave=3, lsm_wg=15, prune_rows=18, prune_wg=27, prune_logits=15, resolve=3), counts
    targets = [c["target"] for c in pm.CASES]
    assert len(targets) == 89 and len(set(targets)) == len(targets), "two matrix cases have the same target"
    want = set(listed) | {("resolve", 0, 1, dt) for dt in pm.DTYPES}
    assert set(targets) == want, (sorted(want - set(targets)), sorted(set(targets) - want))
    assert len({pm.case_id(c) for c in pm.CASES}) == len(targets)
    for c in pm.CASES:
        assert c["target"] in pm.expected_prepass(c).values(), pm.case_id(c)
    # the size bounds of the table are the ones the case table restates (expected_prepass)
    for k, a, b, dt, vmax in table:
        if k in ("lsm_wg", "prune_wg", "prune_logits"):
            assert vmax == {1: 1024, 2: 2048, 4: 4096, 10: 10240, 16: 0}[a], (k, a, vmax)
        elif k == "prune_rows":
            assert vmax == {1: 64, 4: 256, 16: 1024, 64: 4096, 160: 10240, 0: 0}[a], (k, a, vmax)
        else:
            assert vmax == 0, (k, vmax)


def test_python_signature_mirrors_reference():
    import ctcdecode_amd

    sig = inspect.signature(ctcdecode_amd.CTCBeamDecoder.__init__)
    names = list(sig.parameters)[1:11]
    # ctcdecode/__init__.py:26-38 of the reference
    assert names == ["labels", "model_path", "alpha", "beta", "cutoff_top_n", "cutoff_prob", "beam_width", "num_processes", "blank_id", "log_probs_input"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect._empty}
    assert defaults["cutoff_top_n"] == 40 and defaults["cutoff_prob"] == 1.0 and defaults["beam_width"] == 100
    assert defaults["num_processes"] == 4 and defaults["blank_id"] == 0 and defaults["log_probs_input"] is False
    assert list(inspect.signature(ctcdecode_amd.CTCBeamDecoder.decode).parameters) == ["self", "probs", "seq_lens"]


def test_online_signature_mirrors_reference():
    import ctcdecode_amd

    sig = inspect.signature(ctcdecode_amd.OnlineCTCBeamDecoder.__init__)
    assert list(sig.parameters)[1:11] == ["labels", "model_path", "alpha", "beta", "cutoff_top_n", "cutoff_prob", "beam_width", "num_processes", "blank_id", "log_probs_input"]
    # ctcdecode/__init__.py:189
    dsig = inspect.signature(ctcdecode_amd.OnlineCTCBeamDecoder.decode)
    assert list(dsig.parameters)[:5] == ["self", "probs", "states", "is_eos_s", "seq_lens"]
    # (extensions come after the reference's parameters and have defaults that keep the reference's behaviour: check=True)
    assert all(p.default is not inspect._empty for p in list(dsig.parameters.values())[5:]) and dsig.parameters["check"].default is True
    assert list(inspect.signature(ctcdecode_amd.DecoderState.__init__).parameters) == ["self", "decoder"]


def test_product_does_not_touch_the_oracle():
    """The product path must never import/load anything under oracle/ (it is test infrastructure)."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "ctcdecode_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle/" not in text.replace("oracle/ (", "").replace("under oracle/", "") or f == "__init__.py", f
                assert "libctcoracle" not in text and "libctcref" not in text, f


def test_reference_import_name():
    """README.md:22-38 of the reference: ``from ctcdecode import CTCBeamDecoder`` (+ the online classes) works unchanged."""
    import ctcdecode
    import ctcdecode_amd

    assert ctcdecode.CTCBeamDecoder is ctcdecode_amd.CTCBeamDecoder
    assert ctcdecode.OnlineCTCBeamDecoder is ctcdecode_amd.OnlineCTCBeamDecoder and ctcdecode.DecoderState is ctcdecode_amd.DecoderState


def test_destructors_inside_a_scorer_callback_are_queued():
    """_native.destroy: a ctcd_*_destroy asked for while a scorer callback runs (the collector ran a destructor there) frees HBM and
    would wait for the launch that waits for the callback; it is queued, and the next checked call outside a callback makes it --
    in the order the destructors ran (a stream before its decoder).  test_gpu_lm.py holds the decode that does this on the device."""
    from ctcdecode_amd import _native

    calls = []
    assert _native._in_callback == 0 and _native._deferred == []
    _native._in_callback += 1
    try:
        _native.destroy(lambda *h: calls.append(h), "decoder", "stream")
        _native.destroy(lambda *h: calls.append(h), "decoder")
        _native.check(0)  # (a checked call inside the callback: still queued)
        assert calls == [] and len(_native._deferred) == 2
    finally:
        _native._in_callback -= 1
    _native.check(0)
    assert calls == [("decoder", "stream"), ("decoder",)] and _native._deferred == []
    _native._in_callback += 1
    try:
        _native.destroy(lambda *h: calls.append(h), "first")
    finally:
        _native._in_callback -= 1
    _native.destroy(lambda *h: calls.append(h), "second")  # (outside a callback: at once, behind what was queued)
    assert calls[2:] == [("first",), ("second",)] and _native._deferred == []
