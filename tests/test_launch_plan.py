"""The host's choice of the decode kernel (ctcdecode_amd/csrc/launch_plan.h plan_launch) on the CPU, through the core's host build: every
case of the kernel matrix plans the kernel its GPU test launches (tests/test_gpu_kernel_matrix.py), and the capability limits of
tests/test_gpu_decode.py::test_capability_boundaries fall where the GPU finds them."""
import ctypes
import os

import numpy as np
import pytest

import kernel_matrix_util as km
import oracle_util as ou
import prepass_matrix_util as pm

CU_COUNT = 256  # (above every case's B: the automatic two-workgroups-per-CU choice stays off unless a check asks for it)
EUNSUPPORTED = -2  # include/ctcdecode_amd.h CTCD_EUNSUPPORTED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the product build's CTC_KERNEL_LIST: the kernels the planner may choose
LISTED = np.ascontiguousarray(km.parse_kernel_list(open(os.path.join(ROOT, "ctcdecode_amd", "csrc", "decode_kernel.h")).read()), np.int32)


def plan(V, K, top_n=40, cutoff_prob=1.0, B=2, threads=0, fixed=True, profile=0, cu_sharing=-1, subtree=-1, subtree_on=False, scorer=0,
         streamed=False):
    """-> (rc, (PROF, BIG, LAYOUT, PRUNED, NT, LM, OCC2), layout) of a call; profile 2 = the barrier timeline armed."""
    lib = ctypes.CDLL(ou.build_core_host())
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.ctccore_plan_kernel.argtypes = [i32p] + [ctypes.c_int] * 5 + [ctypes.c_double] + [ctypes.c_int] * 11 + [i32p]
    out = (ctypes.c_int32 * 10)()
    rc = lib.ctccore_plan_kernel(LISTED.ctypes.data_as(i32p), len(LISTED), B, V, K, top_n, cutoff_prob, threads, pm.LDS_BYTES, CU_COUNT,
                                 int(not fixed), int(profile > 0), int(profile == 2), cu_sharing, subtree, int(subtree_on), scorer,
                                 int(streamed), out)
    return rc, tuple(out[:7]), out[7]


@pytest.mark.parametrize("c", km.CASES, ids=km.case_id)
def test_plan_matches_kernel_matrix(c):
    rc, key, layout = plan(c["V"], c["K"], c["top_n"], c["cutoff_prob"], B=c["B"], threads=c["threads"] or 0, fixed=c["fixed"],
                           profile=c["profile"], cu_sharing=c["cu_sharing"], subtree=c["subtree"], scorer=km.scorer_kind(c),
                           streamed=c["streamed"])
    assert rc == 0, rc
    assert key == c["kernel"]
    assert layout == km.expected_layout(c["kernel"])


def test_plan_automatic_choices():
    """Two workgroups per CU and the subtree search: automatic (-1), forced on, and where they never apply."""
    north = dict(V=29, K=100, threads=1024)
    assert plan(**north, B=CU_COUNT)[1] == (0, 0, 1, 0, 1024, 0, 0)
    assert plan(**north, B=CU_COUNT + 1)[1] == (0, 0, 1, 0, 1024, 0, 1)
    assert plan(**north, B=CU_COUNT + 1, cu_sharing=0)[1] == (0, 0, 1, 0, 1024, 0, 0)
    assert plan(**north, subtree_on=True)[1] == (3, 0, 1, 0, 1024, 0, 0)
    assert plan(**north, subtree_on=True, subtree=0)[1] == (0, 0, 1, 0, 1024, 0, 0)
    assert plan(**north, subtree_on=True, B=CU_COUNT + 1)[1] == (0, 0, 1, 0, 1024, 0, 1)  # (the two exclude each other)
    # the instrumented builds and the scorer hook run one workgroup per CU, even on request
    assert plan(V=29, K=64, profile=1, cu_sharing=1)[1] == (1, 0, 1, 0, 0, 0, 0)
    assert plan(V=29, K=64, profile=2, threads=1024, cu_sharing=1)[1] == (2, 0, 1, 0, 1024, 0, 0)
    assert plan(V=29, K=48, scorer=3, cu_sharing=1)[1] == (0, 0, 1, 0, 1024, 3, 0)
    # the subtree search is a build of the scorer-free fixed layout at 1024 threads
    assert plan(V=29, K=48, scorer=2, subtree=1)[1] == (0, 0, 1, 0, 1024, 2, 0)
    assert plan(V=29, K=50, threads=512, subtree=1)[1] == (0, 0, 1, 0, 0, 0, 0)


def test_plan_capability_boundaries():
    """The CTCD_EUNSUPPORTED edges of test_capability_boundaries that are the planner's, and the layouts on their supported side."""
    # more than 65535 candidate slots (66 * 1002): workspace level 3
    rc, _, layout = plan(1000, 65, 1000)
    assert rc == 0 and layout != 6
    assert plan(1000, 66, 1000)[::2] == (0, 6)
    # one workgroup's LDS: beam 1000 at HBM level 2, beam 1400 beyond it
    assert plan(29, 1000)[::2] == (0, 5)
    assert plan(29, 1400)[0] == EUNSUPPORTED
    # 16 777 215 candidate slots; pruning with more than 32767 labels
    assert plan(60000, 300, 60000)[0] == EUNSUPPORTED
    assert plan(40000, 4, 40)[0] == EUNSUPPORTED
    assert plan(32767, 4, 40)[0] == 0
