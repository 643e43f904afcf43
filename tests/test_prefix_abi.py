"""CPU-side checks of the prefix scores' C ABI: the names are bound, and the entry points refuse a NULL decoder before anything else."""
import pytest


def test_prefix_entry_points_are_bound_and_refuse_a_null_decoder():
    import __graft_entry__ as g

    g.build()
    from ctcdecode_amd import _native

    lib, n = _native.lib, None
    assert {"ctcd_ctc_prefix_init", "ctcd_ctc_prefix_scores", "ctcd_ctc_prefix_advance", "ctcd_last_prefix_kernel"} <= set(_native.SYMBOLS) and lib.ctcd_last_prefix_kernel(n) == -1
    for call in (lambda: lib.ctcd_ctc_prefix_init(n, n, n, 1, 1, 2, 0, 1, 1, n, n, n, n),
                 lambda: lib.ctcd_ctc_prefix_scores(n, n, n, 1, 1, 2, 0, 1, n, n, n, 1, n, 0, n, n, n, n),
                 lambda: lib.ctcd_ctc_prefix_advance(n, n, n, 1, 1, 2, 0, 1, n, n, n, 1, n, n, 1, n, n, n, n, n)):
        with pytest.raises(ValueError, match="decoder == NULL"):
            _native.check(call())
