"""The kRandomNodes fan-out graph build (rf_scatter / rf_rows, on a shard rfx_soff / rfx_meta / rfx_index) row by row against the
draw: the test hook sim_t_rf_graph runs the handle's own build for any tick and copies the graph out, tests/graph_model.py says
what it has to hold.  Exact comparisons, no protocol run (but for the tests that show the hook is neutral and the receiving side's
cells are the oracle's packets).  Every case asserts from the hook's figures (`info`) that it drove the path it means to drive."""
import ctypes as C
import time

import numpy as np
import pytest

from serf_amd import _ffi
from tests import _scenario as sc
from tests import graph_model as gm

pytestmark = pytest.mark.gpu

SEED = _ffi.DEFAULT_SEED
TICKS = (0, 1, 7, (1 << 21) + 5)
RF = _ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT
INFO = ("LB", "PB", "NB", "NBh", "cap", "bcap", "wide", "lean", "NWG", "cnt_u", "tot_u", "cell_u", "slab_u", "slab_cap", "max_bucket", "overflow")
RFR, RF_EPT = 512, 24   # threads of an rf_rows workgroup, pairs a thread keeps (serf_sim_kernels.inc)
ENV = ("SERF_RF_LB", "SERF_RF_CAP", "SERF_RF_BCAP", "SERF_RF_WIDE", "SERF_RF_SYNC")


def _env(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in kw.items():
        if v is not None:
            monkeypatch.setenv("SERF_RF_" + k.upper(), str(v))


def rf_graph(hiplib, sim, tick, which=0):
    """sim_t_rf_graph: (the words it wrote, info as a dict, seconds it took)."""
    fn = hiplib.dll.sim_t_rf_graph
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    cfg = sim.cfg
    n, V, Cn = int(cfg.n_nodes), int(cfg.vshards), max(1, int(cfg.chunks))
    nl = n // V if int(cfg.shard_count) > 1 else n
    out = np.zeros(6 * nl + Cn * (n // 4 + 4400) + 8192, np.uint32)
    info = (C.c_uint32 * 16)()
    t0 = time.perf_counter()
    words = fn(sim.h, tick, which, out.ctypes.data, out.size, info)
    dt = time.perf_counter() - t0
    assert words >= 0, f"sim_t_rf_graph returned {words}"
    return out[:words].astype(np.int64), dict(zip(INFO, info)), dt


def _same(got, want, what, name=lambda i: f"element {i}"):
    assert len(got) == len(want), f"{what}: {len(got)} entries, the model has {len(want)}"
    bad = np.nonzero(np.asarray(got, np.int64) != np.asarray(want, np.int64))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: {name(i)}: {got[i]} where the model has {want[i]} ({len(bad)} differ)")


def check_one_handle(hiplib, sim, n, fanout, tick, what):
    feff = gm.feff_of(n, fanout)
    out, info, dt = rf_graph(hiplib, sim, tick)
    rcsr, rsrc = gm.one_handle(int(sim.cfg.seed), tick, n, feff)
    _same(out[:n + 1], rcsr, f"{what} tick {tick} rcsr", lambda i: f"row {i}")
    _same(out[n + 1:], rsrc, f"{what} tick {tick} rsrc", lambda i: f"row {int(np.searchsorted(rcsr, i, 'right')) - 1} entry {i}")
    tot = gm.bucket_totals(int(sim.cfg.seed), tick, n, feff, info["LB"])
    assert info["NB"] == len(tot) and info["max_bucket"] == tot.max(initial=0), (what, tick, info)
    assert info["overflow"] == gm.overflow_expected(tot, info["bcap"]), (what, tick, info)
    return info, tot, dt


def one_handle_case(hiplib, monkeypatch, n, fanout, what, ticks=TICKS, **env):
    _env(monkeypatch, **env)
    sim = _ffi.Sim(hiplib, _ffi.make_config(n, fanout=fanout, view_slots=16, event_ring=8, query_ring=8, flags=RF))
    res = [check_one_handle(hiplib, sim, n, fanout, t, what) for t in ticks]
    sim.close()
    print(f"{what}: tick {ticks[0]}: {res[0][0]}")
    return res


# ---- one handle ----
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65])
def test_tiny(hiplib, monkeypatch, n):
    # fewer other nodes than the fan-out: slots without a target; one node: every row empty
    for info, tot, _ in one_handle_case(hiplib, monkeypatch, n, 4, f"n={n}"):
        assert tot.sum() <= n * min(4, n - 1) and (n > 1 or tot.sum() == 0) and info["NB"] == 1 and not info["wide"]


@pytest.mark.parametrize("lb", [8, 9, 10])
@pytest.mark.parametrize("n,fanout", [(256, 4), (257, 4), (3000, 1), (3000, 2), (3000, 3), (3000, 4), (4097, 4), (8193, 4), (8193, 1), (20000, 4)])
def test_lean_rows_by_bucket_width(hiplib, monkeypatch, lb, n, fanout):
    # the instantiation the 1 Mi-node headline runs, at 2^LB <= 1024: full and one-row last buckets, a dozen buckets before a
    # bucket (s_base), scatter workgroups of 4 096 senders and of one; 20 000 nodes at LB = 8: 79 buckets — rf_scatter's prefix over
    # the buckets crosses a wave (one bucket a thread)
    for info, tot, _ in one_handle_case(hiplib, monkeypatch, n, fanout, f"LB={lb} n={n} f={fanout}", lb=lb):
        assert info["LB"] == lb and info["lean"] == 1 and not info["wide"], info
        assert info["NB"] == (n + (1 << lb) - 1) >> lb and info["NWG"] == (n + 4095) // 4096
        assert info["max_bucket"] <= min(info["cap"], info["bcap"]) and info["overflow"] == 0   # LDS ranking, no overflow list


@pytest.mark.parametrize("n,fanout", [(2049, 4), (4097, 1), (4097, 2), (4097, 3), (4097, 4), (20000, 4)])
def test_general_rows_default_width(hiplib, monkeypatch, n, fanout):
    cost = []
    for info, tot, dt in one_handle_case(hiplib, monkeypatch, n, fanout, f"n={n} f={fanout}"):
        assert info["LB"] == 11 and info["lean"] == 0 and not info["wide"], info
        assert info["max_bucket"] <= min(info["cap"], info["bcap"]) and info["overflow"] == 0
        cost.append(dt)
    print(f"LB=11 n={n} f={fanout}: seconds per hook call {cost}")


@pytest.mark.parametrize("lb,n,fanout", [(12, 8193, 1), (12, 8193, 2), (12, 20000, 1), (12, 20000, 2), (12, 20000, 3), (12, 8193, 4), (12, 20000, 4),
                                         (13, 8193, 1), (13, 8193, 2), (13, 20000, 1), (13, 20000, 2)])
def test_wide_buckets(hiplib, monkeypatch, lb, n, fanout):
    # LB = 12 / 13: what create_rf picks for one handle beyond 8 Mi nodes.  cap stops at RF_EPT * RFR = 12 288 pairs, a full bucket
    # holds f << LB on average: 4 096 and 8 192 (LB = 12, f = 1, 2; LB = 13, f = 1) fit; 16 384 (LB = 12, f = 4; LB = 13, f = 2) never
    # does — every full bucket ranks from global memory without being told to —; 12 288 = cap (LB = 12, f = 3): some do, some do not
    cost = []
    mean = fanout << lb
    for info, tot, dt in one_handle_case(hiplib, monkeypatch, n, fanout, f"LB={lb} n={n} f={fanout}", lb=lb):
        assert info["LB"] == lb and info["lean"] == 0 and info["NB"] == (n + (1 << lb) - 1) >> lb, info
        slow = int((tot > info["cap"]).sum())   # the model's buckets that do not fit the build's cap
        assert (info["max_bucket"] > info["cap"]) == (slow > 0), info   # (max_bucket = the model's, check_one_handle)
        if mean <= 8192:
            assert slow == 0 and info["cap"] < RF_EPT * RFR, info   # (the mean and 16 sigma)
        elif mean == 16384:
            assert info["cap"] == RF_EPT * RFR and (tot[:n >> lb] > info["cap"]).all() and slow >= n >> lb > 0, info   # every full bucket
        else:
            assert info["cap"] == RF_EPT * RFR == mean and 0 < slow < info["NB"], info   # both paths in one build
        cost.append((slow, dt))
    print(f"LB={lb} n={n} f={fanout}: (buckets ranked from global memory, seconds per hook call) {cost}")


@pytest.mark.parametrize("lb,n,bcap", [(8, 8193, 1), (8, 8193, 1024), (8, 4097, 1000), (None, 4097, 1), (None, 4097, 8192), (None, 20000, 8100)])
def test_overflow_list(hiplib, monkeypatch, lb, n, bcap):
    # regions of l1 too small for their buckets: the rest goes through the overflow list, from several scatter workgroups
    for info, tot, _ in one_handle_case(hiplib, monkeypatch, n, 4, f"LB={lb} n={n} BCAP={bcap}", lb=lb, bcap=bcap):
        assert info["bcap"] == bcap and info["lean"] == (1 if lb else 0) and info["NB"] > 1 and info["NWG"] > 1, info
        assert info["overflow"] == gm.overflow_expected(tot, bcap) > 0 and info["max_bucket"] <= info["cap"]


@pytest.mark.parametrize("lb,n,cap,fanout", [(8, 3000, 512, 4), (8, 4097, 512, 3), (None, 4097, 1024, 4), (None, 2049, 512, 2)])
def test_slow_path(hiplib, monkeypatch, lb, n, cap, fanout):
    # buckets that do not fit rf_rows' tables rank straight from global memory; CAP = 512 at LB = 8 and fan-out 4: every one of them
    for info, tot, _ in one_handle_case(hiplib, monkeypatch, n, fanout, f"LB={lb} n={n} CAP={cap}", lb=lb, cap=cap):
        assert info["cap"] == cap and info["lean"] == (1 if lb else 0) and info["max_bucket"] > cap and info["overflow"] == 0, info
        if (lb, n) == (8, 3000):
            assert (tot > cap).all()


@pytest.mark.parametrize("lb", [8, None])
@pytest.mark.parametrize("n", [2049, 4097])
def test_wide_entries(hiplib, monkeypatch, lb, n):
    # 64-bit entries: 2 048 senders a scatter workgroup
    for info, tot, _ in one_handle_case(hiplib, monkeypatch, n, 4, f"LB={lb} n={n} WIDE", lb=lb, wide=1):
        assert info["wide"] == 1 and info["NWG"] == (n + 2047) // 2048 and info["lean"] == (1 if lb else 0), info


@pytest.mark.parametrize("lb,n,bcap,cap", [(8, 4097, 1000, 512), (8, 4097, 900, 512), (None, 4097, 8000, 1024)])
def test_wide_overflow_and_slow_path_together(hiplib, monkeypatch, lb, n, bcap, cap):
    # (regions about the mean: the slow path walks the overflow list once for every entry beyond a region and every pair it ranks)
    for info, tot, _ in one_handle_case(hiplib, monkeypatch, n, 4, f"LB={lb} n={n} WIDE BCAP={bcap} CAP={cap}",
                                        lb=lb, wide=1, bcap=bcap, cap=cap):
        assert info["wide"] == 1 and info["cap"] == cap and info["bcap"] == bcap and info["lean"] == (1 if lb else 0), info
        assert info["max_bucket"] > cap and info["overflow"] == gm.overflow_expected(tot, bcap) > 0


@pytest.mark.parametrize("rf_sync", [None, 1])
def test_the_hook_is_neutral(oracle, hiplib, monkeypatch, rf_sync):
    # a run with SWIM and loss against the oracle while the hook overwrites graph buffers between the ticks — the one the next tick
    # reads (tick - 1, tick + 5: the same buffer), the two the look-ahead has queued (tick, tick + 1): the schedule builds again
    # whatever it needs, every digest is the oracle's
    n, fanout = 3000, 4
    _env(monkeypatch, lb=8, sync=rf_sync)
    kw = dict(fanout=fanout, view_slots=32, event_ring=16, query_ring=8, probe_interval=3, loss=0.02, push_pull_interval=4, flags=RF)
    g, o = _ffi.Sim(hiplib, _ffi.make_config(n, **kw)), _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    ops = sc.schedule(n, 20, rate=1.0, seed=11, max_member_subjects=12)
    sc.apply_schedule(g, ops)
    sc.apply_schedule(o, ops)
    for t in range(30):
        for tick in (t - 1, t, t + 1, t + 5):
            if tick >= 0:
                info, _, _ = check_one_handle(hiplib, g, n, fanout, tick, f"before tick {t}")
                assert info["LB"] == 8 and info["lean"] == 1
        g.step(1)
        o.step(1)
        assert g.digest() == o.digest(), f"digest differs after tick {t}"
    sc.assert_same_state(g, o, "the hook is neutral")
    g.close()
    o.close()


# ---- a shard ----
def shard_cfg(n, V, Cn, g, fanout=4, **kw):
    return _ffi.make_config(n, vshards=V, shard_rank=g, shard_count=V, chunks=Cn if Cn > 1 else 0, fanout=fanout, **kw)


def check_sending_side(hiplib, sim, n, V, Cn, g, fanout, tick, what):
    """the hook's which = 0 on a shard handle: every chunk's sorted pairs, count bytes, bucket totals, starts, flags"""
    out, info, _ = rf_graph(hiplib, sim, tick)
    M, feff = n // V, gm.feff_of(n, fanout)
    per, cw, nb = fanout * (M // Cn), (n + 3) // 4, info["NB"]
    assert info["NBh"] == (M + (1 << info["LB"]) - 1) >> info["LB"] and nb == V * info["NBh"], info
    assert len(out) == Cn * (per + cw + nb + 2 * V + 2)
    raw = out.astype(np.uint32)
    for c in range(Cn):
        w = f"{what} shard {g} chunk {c} tick {tick}"
        at = c * (per + cw + nb + 2 * V + 2)
        m = gm.sending_side(int(sim.cfg.seed), tick, n, feff, V, Cn, g, c, info["LB"])
        total = int(m["xoff"][V])
        _same(out[at:at + total], m["rsrc"], w + " rsrc", lambda i: f"target {m['t'][i]} entry {i}")
        _same(raw[at + per:at + per + cw].view(np.uint8)[:n], m["cntb"], w + " cntb", lambda i: f"destination {i // M} target {i % M}")
        _same(out[at + per + cw:at + per + cw + nb], m["btot"], w + " btot", lambda i: f"destination {i // info['NBh']} bucket {i % info['NBh']}")
        # (xoff[2 V + 2]: V + 1 starts, V flags; rfx_soff_kernel never writes the last word — padding, not compared)
        xo = out[at + per + cw + nb:at + per + cw + nb + 2 * V + 1]
        _same(xo[:V + 1], m["xoff"], w + " xoff")
        assert not xo[V + 1:].any(), w + ": a slab's overflow flag is up"
        if c == Cn - 1:
            assert info["max_bucket"] == m["btot"].max() and info["overflow"] == gm.overflow_expected(m["btot"], info["bcap"]) == 0, (w, info)
    return info


SHARDS = [(4, 1, 2976), (4, 2, 2976), (3, 1, 2313), (8, 1, 64), (2, 1, 8200)]


@pytest.mark.parametrize("lb", [8, None])
@pytest.mark.parametrize("V,Cn,n", SHARDS)
def test_a_shards_sending_side(hiplib, monkeypatch, lb, V, Cn, n):
    # one shard handle alone, every rank: M = 744 — three buckets per destination at LB = 8, the last of 232 rows —; M = 771, odd:
    # count sections that start off alignment, a last bucket of 3 rows; M = 8; M = 4 100: 17 buckets per destination, two of 2 048
    _env(monkeypatch, lb=lb)
    M = n // V
    for g in range(V):
        sim = _ffi.Sim(hiplib, shard_cfg(n, V, Cn, g, view_slots=16 if n > 64 else 0, event_ring=8, query_ring=8, flags=RF))
        for tick in TICKS:
            info = check_sending_side(hiplib, sim, n, V, Cn, g, 4, tick, f"V={V} C={Cn} n={n} LB={lb}")
            assert info["LB"] == (lb or 11) and not info["wide"] and info["NBh"] == (M + (1 << info["LB"]) - 1) >> info["LB"], info
            assert info["lean"] == (1 if lb else 0), info
        sim.close()
    print(f"V={V} C={Cn} n={n} LB={lb}: last shard, tick {TICKS[-1]}: {info}")


@pytest.mark.parametrize("V,Cn,n,fanout", [(4, 1, 2976, 1), (4, 2, 2976, 3), (3, 1, 2313, 2)])
def test_a_shards_sending_side_other_fanouts(hiplib, monkeypatch, V, Cn, n, fanout):
    _env(monkeypatch, lb=8)
    for g in (0, V - 1):
        sim = _ffi.Sim(hiplib, shard_cfg(n, V, Cn, g, fanout=fanout, view_slots=16, event_ring=8, query_ring=8, flags=RF))
        for tick in TICKS:
            check_sending_side(hiplib, sim, n, V, Cn, g, fanout, tick, f"V={V} C={Cn} n={n} f={fanout}")
        sim.close()


@pytest.mark.parametrize("V,Cn,n", [(4, 1, 2976), (4, 2, 2976), (3, 1, 2313)])
def test_a_shards_receiving_side_and_the_slabs(oracle, hiplib, monkeypatch, V, Cn, n):
    # V shard handles on one GPU, device copies for the exchange (tests/test_parity_gpu.py), LB = 8: ragged last buckets on both
    # sides, rfx_meta's byte path (M % 16 != 0), count sections off alignment (M odd), (nrows + 3) / 4 with nrows % 4 != 0.  After
    # every tick: every slab's header, count bytes and bucket totals in the send tensors = the model's sending side of that tick;
    # every shard's rx_rcsr / rx_rsrc = the model's receiving side of the tick before (what the tick just run read); the state
    # arrays = the oracle's slices (the cells' contents)
    import torch

    from tests.test_parity_gpu import _packed_exchange_chunk_on_one_gpu, _push_pull_on_one_gpu, _suspicions_on_one_gpu

    _env(monkeypatch, lb=8)
    M, fanout, feff, ticks = n // V, 4, 4, 20
    kw = dict(fanout=fanout, view_slots=96, event_ring=16, query_ring=8, leave_delay=6, probe_interval=4, loss=0.02, push_pull_interval=3, flags=RF)
    ref = _ffi.Sim(oracle, _ffi.make_config(n, vshards=V, **kw))
    shards, send, recv = [], [], []
    for g in range(V):
        s = _ffi.Sim(hiplib, shard_cfg(n, V, Cn, g, **kw))
        kind, planes, pb, rb = s.exchange_layout()
        assert kind == _ffi.XCHG_PACKED and pb == rb
        send.append(torch.zeros(pb, dtype=torch.uint8, device="cuda"))
        recv.append([torch.zeros(rb, dtype=torch.uint8, device="cuda") for _ in range(2 if Cn > 1 else 1)])
        s.bind_exchange3(send[-1].data_ptr(), pb, recv[-1][0].data_ptr(), recv[-1][-1].data_ptr(), rb)
        shards.append(s)
    ops = sc.schedule(n, ticks // 2, rate=0.8, seed=5, max_member_subjects=40)
    for s in shards + [ref]:
        sc.apply_schedule(s, ops)
    _, L, _ = rf_graph(hiplib, shards[0], 0, which=1)
    nbh = (M + 255) >> 8
    assert L["LB"] == 8 and L["NBh"] == nbh and L["lean"] == 1 and M % 16 != 0 and (M - ((nbh - 1) << 8)) < 256
    assert L["tot_u"] == 1 + (M + 63) // 64 and L["cell_u"] == L["tot_u"] + (nbh + 15) // 16 and pb == Cn * V * L["slab_u"] * 64
    PG = (L["slab_u"] - L["cell_u"]) // L["slab_cap"]
    print(f"V={V} C={Cn} n={n}: {L}")
    for t in range(ticks):
        for s in shards:
            s.step_begin()
        if shards[0].pp_due():
            _push_pull_on_one_gpu(shards)
        into = [r[t & 1] if Cn > 1 else r[0] for r in recv]
        for c in range(Cn):
            for s in shards:
                s.step_chunk(c)
                s.sync()
            _packed_exchange_chunk_on_one_gpu(send, into, c, Cn)
        for s in shards:
            s.step_end()
            s.sync()
        _suspicions_on_one_gpu(shards)
        torch.cuda.synchronize()
        ref.step(1)
        for s in range(V):   # the slabs shard s has just packed
            buf = send[s].cpu().numpy()
            for c in range(Cn):
                for g in range(V):
                    slab = buf[(c * V + g) * L["slab_u"] * 64:(c * V + g + 1) * L["slab_u"] * 64]
                    hdr, cb, bt = gm.slab_meta(SEED, t, n, feff, V, Cn, s, c, g, 8, L["slab_cap"])
                    w = f"tick {t} shard {s} slab ({c}, {g})"
                    assert tuple(int(x) for x in slab[:12].view(np.uint32)) == hdr, w + " header"
                    _same(slab[L["cnt_u"] * 64:L["cnt_u"] * 64 + M], cb, w + " count bytes", lambda i: f"target {i}")
                    _same(slab[L["tot_u"] * 64:L["tot_u"] * 64 + 4 * nbh].view(np.uint32), bt, w + " bucket totals", lambda i: f"bucket {i}")
        for g, s in enumerate(shards):   # the rows tick t read: the packets sent during tick t - 1
            out, _, _ = rf_graph(hiplib, s, 0, which=1)
            if t == 0:
                assert len(out) == M + 1 and not out.any()
                continue
            rcsr, rsrc = gm.receiving_side(SEED, t - 1, n, feff, V, Cn, g, L["slab_u"], L["cell_u"], PG)
            _same(out[:M + 1], rcsr, f"tick {t} shard {g} rx_rcsr", lambda i: f"row {i}")
            _same(out[M + 1:], rsrc, f"tick {t} shard {g} rx_rsrc", lambda i: f"row {int(np.searchsorted(rcsr, i, 'right')) - 1} entry {i}")
        if t % 5 == 2:   # the hook's build on a bound shard between two ticks: the graph ahead, and the one the next pack needs
            for g, s in enumerate(shards):
                for tick in (t + 1, t + 2):
                    check_sending_side(hiplib, s, n, V, Cn, g, fanout, tick, f"between ticks, V={V} C={Cn}")
        if t % 6 == 0 or t == ticks - 1:
            for g, s in enumerate(shards):
                for which in (_ffi.ARR_ROWS, _ffi.ARR_QUEUE):
                    a, b = s.dump(which), ref.dump(which)
                    per = len(b) // n
                    i = sc.first_diff(a, b[g * M * per:(g + 1) * M * per])
                    assert i is None, f"shard {g} array {which} element {i} differs at tick {t}"
                a = s.dump(_ffi.ARR_VIEW).reshape(96, M)
                b = np.ascontiguousarray(ref.dump(_ffi.ARR_VIEW).reshape(96, n)[:, g * M:(g + 1) * M])
                assert a.tobytes() == b.tobytes(), f"shard {g} view differs at tick {t}"
    for s in shards + [ref]:
        s.close()
