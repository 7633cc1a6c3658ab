"""The reference model of the kRandomNodes fan-out graph (tests/graph_model.py) against a brute-force loop over
tests/third_model.py::k_random_nodes, its invariants, its three sharded views as cuts of the one-handle graph — and the test
hook the GPU tests read the build through, present in the library without being part of the declared ABI.  No device."""
import ctypes as C

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import graph_model as gm
from tests import third_model as tm

SEED = _ffi.DEFAULT_SEED
SIZES = (1, 2, 3, 5, 257, 3000)
TICKS = (0, 1, 7, (1 << 21) + 5)


def brute_rows(seed, tick, n, feff):
    """row t = every (sender, slot) that drew t, in (sender, slot) order: one plain loop"""
    rows = [[] for _ in range(n)]
    drawn = 0
    for s in range(n):
        for k, t in enumerate(tm.k_random_nodes(seed, tick, s, n, feff)):
            rows[t].append(4 * s + k)
            drawn += 1
    return rows, drawn


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fanout", [1, 4])
def test_rows_against_the_plain_loop(n, fanout):
    feff = gm.feff_of(n, fanout)
    for tick in TICKS if n <= 257 else (7,):
        rows, drawn = brute_rows(SEED, tick, n, feff)
        rcsr, rsrc = gm.one_handle(SEED, tick, n, feff)
        assert rcsr[0] == 0 and rcsr[n] == drawn == len(rsrc)
        for t in range(n):
            assert list(rsrc[rcsr[t]:rcsr[t + 1]]) == rows[t], f"n={n} tick={tick} row {t}"


@pytest.mark.parametrize("n", SIZES)
def test_invariants(n):
    feff = gm.feff_of(n, 4)
    for tick in TICKS:
        tg = gm.k_random_nodes_all(SEED, tick, n, feff)
        rcsr, rsrc = gm.one_handle(SEED, tick, n, feff)
        assert (np.diff(rcsr) >= 0).all() and rcsr[n] == (tg >= 0).sum() == len(rsrc)
        p, _ = gm.pairs_of(tg)
        assert len(np.unique(rsrc)) == len(rsrc) and np.array_equal(np.sort(rsrc), np.sort(p))   # every pair exactly once
        assert ((tg >= 0).sum(axis=1) <= feff).all() and (n < 64 or (tg >= 0).all())   # (3 n draws: a tiny cluster's node may find fewer)
        for t in range(n):
            row = rsrc[rcsr[t]:rcsr[t + 1]]
            assert (np.diff(row) > 0).all() and len(np.unique(row >> 2)) == len(row) and (row >> 2 != t).all(), f"row {t}"
            assert (tg[row >> 2, row & 3] == t).all()


@pytest.mark.parametrize("n,V,C", [(2976, 4, 1), (2976, 4, 2), (2313, 3, 1), (64, 8, 1), (3000, 2, 3)])
def test_the_sharded_views_are_cuts_of_the_graph(n, V, C):
    feff, M, tick, LB = gm.feff_of(n, 4), n // V, 7, 8
    nbh = (M + (1 << LB) - 1) >> LB
    rcsr, rsrc = gm.one_handle(SEED, tick, n, feff)
    slab_u, cell_u = 1 << 20, 17
    rx = [gm.receiving_side(SEED, tick, n, feff, V, C, g, slab_u, cell_u) for g in range(V)]
    snd = {(s, c): gm.sending_side(SEED, tick, n, feff, V, C, s, c, LB) for s in range(V) for c in range(C)}
    # the sending sides: every pair of the graph exactly once, each list sorted by (target, p), counts and totals of that list
    seen = []
    for (s, c), x in snd.items():
        glob = x["rsrc"] + 4 * s * M
        assert ((glob >> 2) // (M // C) == s * C + c).all()
        assert (np.diff(x["t"] * (8 * n) + x["rsrc"]) > 0).all()
        assert np.array_equal(x["cntb"], np.bincount(x["t"], minlength=n)) and x["xoff"][V] == len(glob) == x["btot"].sum()
        for h in range(V):
            assert x["btot"][h * nbh:(h + 1) * nbh].sum() == x["xoff"][h + 1] - x["xoff"][h]
            for b in range(nbh):
                assert x["btot"][h * nbh + b] == x["cntb"][h * M + (b << LB):h * M + min(M, (b + 1) << LB)].sum()
        seen.append(glob)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.sort(rsrc))
    assert np.array_equal(sum(x["cntb"] for x in snd.values()), np.diff(rcsr))
    # the receiving sides: shard g's rows are rows g * M .. of the graph, every entry names the cell its pair was packed into
    for g in range(V):
        rr, rs = rx[g]
        assert np.array_equal(rr, rcsr[g * M:(g + 1) * M + 1] - rcsr[g * M])
        want = rsrc[rcsr[g * M]:rcsr[(g + 1) * M]]
        unit = rs >> 2
        slab, off = unit // slab_u, unit % slab_u - cell_u
        c, s = slab // V, slab % V
        got = np.array([snd[(int(si), int(ci))]["rsrc"][snd[(int(si), int(ci))]["xoff"][g] + o] + 4 * si * M for si, ci, o in zip(s, c, off)],
                       np.int64).reshape(-1)
        assert np.array_equal(got, want), f"shard {g}"
        for (s2, c2), x in snd.items():
            hdr, cb, bt = gm.slab_meta(SEED, tick, n, feff, V, C, s2, c2, g, LB, 1 << 30)
            assert hdr == (x["xoff"][g + 1] - x["xoff"][g], 0, tick) and len(cb) == M and len(bt) == nbh and cb.sum() == bt.sum() == hdr[0]


def test_overflow_and_bucket_totals():
    n, feff, LB = 3000, 4, 8
    tot = gm.bucket_totals(SEED, 1, n, feff, LB)
    assert len(tot) == 12 and tot.sum() == n * feff
    assert gm.overflow_expected(tot, 1) == n * feff - 12 and gm.overflow_expected(tot, int(tot.max())) == 0


def test_the_hook_is_exported_and_undeclared():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    assert hasattr(dll, "sim_t_rf_graph")
    assert "t_rf_graph" not in _ffi.ABI_SYMBOLS and "rf_graph" not in _ffi.ABI_SYMBOLS
    info = (C.c_uint32 * 16)()
    out = (C.c_uint32 * 4)()
    dll.sim_t_rf_graph.restype = C.c_int
    dll.sim_t_rf_graph.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)]
    assert dll.sim_t_rf_graph(None, 0, 0, out, 4, info) == -1   # SIM_EINVAL: no handle, nothing touched
