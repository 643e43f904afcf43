"""The long edit pairs' host code (ctcdecode_amd/csrc/editlong.h) on the CPU: the counts reference against editops_util's, the schedule
walked block by block, and the sequential twin (tests/native/editlong_host.cpp) against the references at the GPU tests' shapes."""
import editdist_util as eu
import editlong_util as lu
import editops_util as ou
import numpy as np
import pytest


def test_the_counts_reference_equals_the_full_matrix_restatement():
    rng = np.random.default_rng(20261126)
    for k in range(200):
        x, y = rng.integers(0, 4 - k % 2 * 2, int(rng.integers(0, 300))), rng.integers(0, 4 - k % 2 * 2, int(rng.integers(0, 300)))
        key, counts, _, _ = ou.align_ref(x, y)
        assert lu.key_ref(x, y) == key == lu.key_ref(y, x) and lu.counts_ref(x, y) == counts, (k, len(x), len(y))
        assert key[0] == eu.lev(x, y)


@pytest.mark.parametrize("W", (2, 4, 16))
@pytest.mark.parametrize("m, n", ((1, 2049), (64, 4097), (65, 10241), (129, 35000), (257, 10241), (321, 10241), (700, 4097), (2112, 6145),
                                  (2113, 10241), (2305, 35000)))
def test_the_schedule_walked_block_by_block(m, n, W):
    """Every block of every tile runs once, on wave tile % W, in order, and so does every row of its right edge.  A load -- from the left
    neighbour's ring or from the slot -- finds, by (tile, row) tags kept per place, that neighbour's row, stored a barrier or more earlier,
    and NO tile (the producer's next, a round later, included) stores to the place in the block of the load.  (m = 1, and 65 with 1 mod
    64, mod 256 and blocks = 2 mod 4 are where a period of a tile's blocks alone goes wrong; m < 2 W x 32 makes the period 2 W.)"""
    G, nb = lu.host_sched(0, 0, m, n, W)[3:5]
    tiles, ring = -(-n // eu.MAX_STRIP), [lu.host_sched(0, 0, m, n, W, r)[8] for r in range(m + 1)]
    assert nb == -(-(m + 63) // 64) and ring == [r % 256 for r in range(m + 1)] and lu.host_sched(0, 0, m, n, W)[9] == -(-4 * (max(m, n) + 1) // 256) * 256
    mem, ran, done, loaded = {}, {}, {}, set()  # place -> tag; tile -> (its last block, when); tag -> the global block that stored it
    for g in range(G + 1):
        loads, stores = [], {}
        for w in range(W):
            active, k, j = lu.host_sched(g, w, m, n, W)[:3]
            if not active:
                continue
            assert g < G and k % W == w and (ran[k] == (j - 1, g - 1) if j else k not in ran), (g, w, k, j)
            ran[k] = (j, g)
            first, rows_done, edge = lu.host_sched(g, w, m, n, W, j)[5:8]
            if k > 0:
                loads += [((w - 1, ring[r]) if w else ("slot", r), (k - 1, r)) for r in range(first, min(first + 63, m) + 1)]
            for r in range(max(edge, 1), min(edge + 63, m) + 1):  # lane 63 completes a row per step
                assert (k, r) not in done and r <= rows_done
                done[(k, r)] = g
                if k + 1 < tiles:
                    stores[(w, ring[r]) if w + 1 < W else ("slot", r)] = (k, r)
            assert rows_done == min(edge + 63, m)
        for place, tag in loads:
            assert mem.get(place) == tag and done.get(tag, G) < g and place not in stores and tag not in loaded, (g, place, tag, mem.get(place))
            loaded.add(tag)
        mem.update(stores)
    assert ran == {k: (nb - 1, ran[k][1]) for k in range(tiles)} and max(v[1] for v in ran.values()) == G - 1 and len(done) == tiles * m and len(loaded) == (tiles - 1) * m


@pytest.mark.parametrize("W", (2, 4, 16))
@pytest.mark.parametrize("n", lu.STRIPS)
def test_the_twin_equals_the_references(n, W):
    c = lu.strip_case(n)
    for k in range(len(c["dist"])):  # both roles for the counts (DISJOINT: one role)
        x, y = c["x"][k, 0, :c["x_lens"][k, 0]], c["y"][k, 0, :c["y_lens"][k, 0]]
        H, S, Del, I = (int(v) for v in c["counts"][k])
        assert lu.host_pair(x, y, W, False) == c["dist"][k] and lu.host_pair(x, y, W, True) == (H, S, Del, I), (n, k)
        assert len(y) in lu.DISJOINT or lu.host_pair(y, x, W, True) == (H, S, I, Del), (n, k)
