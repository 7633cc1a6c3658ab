"""The traffic meter of the HIP library (include/serf_sim_traffic.h) against the reference model (tests/traffic_model.py) on the
oracle, run side by side with it: behind every step every word of every sample, the whole map through traffic_nodes,
traffic_top for every column and traffic_summary for every column are compared exactly.  The scenarios are those of
tests/test_traffic.py; the shapes are the observer shapes of tests/test_observer_shapes.py — ragged, tiny, idle, and one size
beyond what one pass of the capped grid covers (traffic_send_kernel, traffic_recv_kernel and traffic_stat_kernel have the
series' pass loop and grid cap).  Then the sampling rules, the errors, a meter across sim_restore, and neutrality: the digests
of a run with the meter equal those of the run without it and the oracle's.  Every call goes through Sim.traffic_*: a library
without the symbols fails these tests, it does not skip them."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from serf_amd.workload import apply_schedule
from tests import series_model
from tests import test_observer_shapes as shapes
from tests import test_traffic as tt
from tests.traffic_model import TrafficModel

pytestmark = pytest.mark.gpu
COLS = range(_ffi.TRAFFIC_COLUMNS)
TRAFFIC_GRID = tt.TRAFFIC_GRID


def words(a):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(a))).view(np.uint64).reshape(-1)


def same_records(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} != {want.shape}"

    def walk(g, w, path):
        if w.dtype.names:
            for f in w.dtype.names:
                walk(g[f], w[f], f"{path}.{f}")
            return
        bad = np.argwhere(np.asarray(g != w))
        assert not len(bad), f"{what}: {path} at {bad[0].tolist()}: HIP {np.asarray(g)[tuple(bad[0])]} != model {np.asarray(w)[tuple(bad[0])]}"
    walk(got, want, "")
    assert got.tobytes() == want.tobytes(), what


def same_reads(g, m, what, top_ks=(10,), widths=(1, 3)):
    """The samples, the whole map, a slice of it, the ranking and the summary of every column."""
    n = int(g.cfg.n_nodes)
    assert g.traffic_count() == m.count(), what
    same_records(g.traffic_read(), m.read(), f"{what}: samples")
    same_records(g.traffic_nodes(), m.nodes(), f"{what}: the map")
    if n > 5:
        same_records(g.traffic_nodes(2, 3), m.nodes(2, 3), f"{what}: nodes 2 .. 4")
        assert len(g.traffic_nodes(n, 0)) == 0
    for c in COLS:
        for k in top_ks:
            same_records(g.traffic_top(k, c), m.top(k, c), f"{what}: top {k} by column {c}")
        for bw in widths:
            same_records(np.atleast_1d(g.traffic_summary(c, bw)), np.atleast_1d(m.summary(c, bw)), f"{what}: summary of column {c}, bin_width {bw}")


def pair(n, kw, ops):
    """A fresh oracle with its model and a fresh HIP handle, the schedule injected into both."""
    o = tt.make(n, kw)
    g = serf_amd.create(n, **kw)
    apply_schedule(o, ops)
    apply_schedule(g, ops)
    return o, TrafficModel(o), g


def side_by_side(n, kw, ops, ticks, what, chunk=1, check=None, **start):
    """Both sides started alike and stepped `chunk` ticks at a time, everything compared behind every step; at the end the
    rankings of 1 and 64 as well, the digest, and check(o, m) — that the scenario moved what it is for."""
    o, m, g = pair(n, kw, ops)
    start = dict(dict(first_tick=0, period=1, capacity=ticks), **start)
    m.start(**start)
    g.traffic_start(**start)
    for t in range(0, ticks, chunk):
        m.step(min(chunk, ticks - t))
        g.step(min(chunk, ticks - t))
        same_reads(g, m, f"{what}, tick {o.tick}")
    same_reads(g, m, f"{what}, the end", top_ks=(1, 64), widths=(7,))
    assert g.digest() == o.digest(), what
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0, "the run stays inside the model's bounds"
    if check:
        check(o, m)
    g.close()
    o.close()


# ---- 1. shapes ----
@pytest.mark.parametrize("fan", sorted(tt.FANOUTS))
@pytest.mark.parametrize("n", shapes.RAGGED_SIZES)
def test_ragged_sizes(hiplib, n, fan):
    """20 ticks of the small churn schedule.  At 1, 2 and 3 nodes there are fewer other nodes than the fan-out: slots without a
    target, rows of the graph that are empty."""
    def check(o, m):
        s = m.read()
        assert s["degree_bins"].sum(axis=1).tolist() == [n] * tt.CHURN_TICKS and (s["record_bins"].sum(axis=1) == s["packets"]).all()
        if n == 1:
            assert not s["packets"].any() and not m.map.any()
        else:
            assert s["packets"].sum() > 0
            if fan == "bijection" or n <= 3:
                assert s["max_packets"].max() <= min(n - 1, tt.FANOUT)
        if n >= 63:
            assert m.nodes()["rx_down"].sum() == s["to_down"].sum() > 0 and s["running"].min() < n, "crashes: rx_down moves"
            assert s["max_packets"].max() > tt.FANOUT or fan == "bijection"
    side_by_side(n, tt.churn_kw(n, fan), tt.churn_ops(n), tt.CHURN_TICKS, f"ragged({n}) {fan}", check=check)


@pytest.mark.parametrize("fan", sorted(tt.FANOUTS))
def test_multi_page_packets_257_nodes(hiplib, fan):
    """pkt_records = 16: packets of up to four pages; the records field (5 bits) and the units field (7 bits) at their largest."""
    def check(o, m):
        s = m.read()
        assert s["packet_records_max"].max() == 16 and s["packet_units_max"].max() == 87 and s["record_bins"][:, 15].sum() > 0
    side_by_side(257, tt.churn_kw(257, fan, **tt.PKT16), tt.churn_ops(257, burst=tt.PKT16_BURST), tt.CHURN_TICKS, f"pkt16 {fan}", check=check)


@pytest.mark.parametrize("fan", sorted(tt.FANOUTS))
def test_loss_1000_nodes(hiplib, fan):
    def check(o, m):
        s = m.read()
        assert (s["packets"] < s["senders"] * tt.FANOUT).any(), "loss removed packets of nodes that sent others"
    side_by_side(1000, tt.churn_kw(1000, fan, loss=0.3), tt.churn_ops(1000), tt.CHURN_TICKS, f"loss {fan}", check=check)


@pytest.mark.parametrize("fan", sorted(tt.FANOUTS))
def test_swim_layer_1025_nodes(hiplib, fan):
    """probe_interval = 5: ALIVE / SUSPECT / DEAD records (kinds 5 - 7) and their lengths among the packets."""
    def check(o, m):
        assert m.read()["to_down"].sum() > 0
    kinds = []
    o = tt.make(1025, tt.churn_kw(1025, fan, probe_interval=5))
    apply_schedule(o, tt.churn_ops(1025))
    for _ in range(tt.CHURN_TICKS):
        o.step(1)
        kinds.append(series_model.sample(o)[45:48])
    o.close()
    assert np.array(kinds).sum(axis=0).min() > 0, "records of kinds 5, 6 and 7 travel in this run"
    side_by_side(1025, tt.churn_kw(1025, fan, probe_interval=5), tt.churn_ops(1025), tt.CHURN_TICKS, f"swim {fan}", check=check)


def test_vshards_2048_nodes_bijection(hiplib):
    """vshards = 4 on one handle that holds every node: the bijection's inverse across virtual shards."""
    side_by_side(2048, tt.churn_kw(2048, "bijection", vshards=4), tt.churn_ops(2048), tt.CHURN_TICKS, "vshards 4")


@pytest.mark.parametrize("fan", sorted(tt.FANOUTS))
@pytest.mark.parametrize("n", shapes.IDLE_SIZES)
def test_nobody_runs(hiplib, n, fan):
    """Every node crashes at tick 5: behind that everything of a sample is zero and the in-degree bins still sum to n_nodes."""
    ops = [(0, _ffi.OP_USER_EVENT, 0, 0x77, 64)] + [(shapes.IDLE_CRASH, _ffi.OP_CRASH, x, 0, 0) for x in range(n)]

    def check(o, m):
        s = m.read()
        assert s["running"].tolist() == [n] * shapes.IDLE_CRASH + [0] * (shapes.IDLE_TICKS - shapes.IDLE_CRASH)
        late = words(s[shapes.IDLE_CRASH + 1:]).reshape(-1, _ffi.TRAFFIC_WORDS)
        assert not late[:, 1:14].any() and not late[:, 17:].any() and (late[:, 16] == n).all() and late[:, 14].tolist() == list(range(shapes.IDLE_CRASH + 2, shapes.IDLE_TICKS + 1))
        if n > 1:
            assert s["packets"][:shapes.IDLE_CRASH].sum() > 0
    side_by_side(n, tt.churn_kw(n, fan), ops, shapes.IDLE_TICKS, f"nobody_runs({n}) {fan}", check=check)


SECOND_N, SECOND_TICKS, SECOND_PERIOD = TRAFFIC_GRID * shapes.BLOCK + shapes.SECOND_PASS, 9, 4


def test_second_pass(hiplib):
    """TRAFFIC_GRID * BLOCK + 65 nodes: the pass loops of the send, receive and summary kernels take a second turn, of one whole
    wave and one lane; the event's origin and the crashed node lie in that pass.  Compared behind every sample."""
    n = SECOND_N
    tt.test_the_cap_is_the_sources()
    assert n == shapes.SERIES_N == 262209

    def check(o, m):
        s, nodes = m.read(), m.nodes()
        assert s["tick"].tolist() == [1, 5, 9] and s["running"].tolist() == [n, n - 1, n - 1]
        assert nodes["tx_packets"][n - 3] > tt.FANOUT, "the origin, a node of the second pass, sent in more than one sample"
        assert nodes["tx_packets"][:TRAFFIC_GRID * shapes.BLOCK].sum() > 0 and nodes["rx_packets"][TRAFFIC_GRID * shapes.BLOCK:].sum() > 0
    kw = dict(shapes.BIG_KW)
    ops = [(2, _ffi.OP_CRASH, n - 1, 0, 0), (0, _ffi.OP_USER_EVENT, n - 3, shapes.EVENT_KEY, 64)]
    side_by_side(n, kw, ops, SECOND_TICKS, "second pass", chunk=SECOND_PERIOD, check=check, period=SECOND_PERIOD, capacity=8)


# ---- 2. sampling ----
def test_period_3_from_tick_5_a_full_buffer_and_a_restart(hiplib):
    """Samples behind ticks 5, 8, 11, 14; the fifth that is due finds the buffer full: counted, nothing accumulated.  Then stop and
    start again: the map is zero again."""
    n, kw = 257, tt.churn_kw(257, "krandomnodes")
    o, m, g = pair(n, kw, tt.churn_ops(n))
    for s in (m, g):
        (s.start if s is m else s.traffic_start)(first_tick=5, period=3, capacity=4)
    m.step(tt.CHURN_TICKS)
    g.step(tt.CHURN_TICKS)                                                 # ONE call
    assert g.traffic_count() == m.count() == (4, 1) and g.traffic_read()["tick"].tolist() == [6, 9, 12, 15]
    same_reads(g, m, "period 3 from tick 5, a full buffer", top_ks=(1, 10, 64))
    assert g.traffic_nodes()["tx_packets"].sum() == g.traffic_read()["packets"].sum() and g.traffic_summary(0)["samples"] == 4
    m.stop()
    g.traffic_stop()
    assert g.traffic_count() == (0, 0)
    m.start(0, 1, 8)
    g.traffic_start(0, 1, 8)
    assert not words(g.traffic_nodes()).any() and g.traffic_summary(3)["bins"][0] == n
    m.step(3)
    g.step(3)
    assert g.traffic_read()["samples"].tolist() == [1, 2, 3]
    same_reads(g, m, "started again", top_ks=(1, 10, 64))
    assert g.digest() == o.digest()
    g.close()
    o.close()


def test_one_step_call_against_single_steps_with_reads_between(hiplib):
    """sim_step(h, 20) against twenty sim_step(h, 1) with every read of the map between them: a read changes nothing."""
    n, kw = 1000, tt.churn_kw(1000, "bijection")
    a, b = serf_amd.create(n, **kw), serf_amd.create(n, **kw)
    for s in (a, b):
        apply_schedule(s, tt.churn_ops(n))
        s.traffic_start(0, 1, tt.CHURN_TICKS)
    a.step(tt.CHURN_TICKS)
    for _ in range(tt.CHURN_TICKS):
        b.step(1)
        b.traffic_nodes(1, 5), b.traffic_top(3, 6), b.traffic_summary(2, 5), b.traffic_read(0, 1)
    same_records(a.traffic_read(), b.traffic_read(), "step(20) against 20 step(1)")
    same_records(a.traffic_nodes(), b.traffic_nodes(), "step(20) against 20 step(1): the map")
    a.close()
    b.close()


# ---- 3. neutrality ----
@pytest.mark.parametrize("fan", sorted(tt.FANOUTS))
def test_digests_with_and_without_the_meter(hiplib, fan):
    n, ticks, kw = 1000, 40, tt.churn_kw(1000, fan, probe_interval=5, loss=0.01)
    ops = tt.churn_ops(n, ticks)
    o = tt.make(n, kw)
    with_meter, without = serf_amd.create(n, **kw), serf_amd.create(n, **kw)
    for s in (o, with_meter, without):
        apply_schedule(s, ops)
    with_meter.traffic_start(0, 1, ticks)
    for s in (o, with_meter, without):
        s.step(ticks)
    assert with_meter.traffic_count() == (ticks, 0) and with_meter.traffic_read()["packets"].sum() > 0
    assert with_meter.digest() == without.digest() == o.digest()
    assert with_meter.snapshot().tobytes() == without.snapshot().tobytes(), "an image holds no meter"
    assert without.traffic_count() == (0, 0)
    for s in (o, with_meter, without):
        s.close()


# ---- 4. errors and states ----
def test_errors_leave_everything_as_it_was(hiplib):
    n, kw = 257, tt.churn_kw(257, "krandomnodes")
    every = lambda s: (lambda: s.traffic_start(0, 1, 8), s.traffic_count, lambda: s.traffic_read(0, 0), s.traffic_stop,
                       lambda: s.traffic_nodes(0, 1), lambda: s.traffic_top(3, 0), lambda: s.traffic_summary(0, 1))
    sh = serf_amd.create(n, force_sharded=True, **kw)                     # a shard has no meter
    for call in every(sh):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    o, m, g = pair(n, kw, tt.churn_ops(n))
    assert g.traffic_count() == (0, 0)
    for call in every(g)[2:]:                                              # no meter yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    for args in ((0, 0, 8), (0, 1, 0), (0, 1, _ffi.TRAFFIC_MAX_SAMPLES + 1)):
        with pytest.raises(_ffi.SimError) as ei:
            g.traffic_start(*args)
        assert ei.value.code == _ffi.EINVAL and g.traffic_count() == (0, 0)
    f, u, ref = g.lib.f, _ffi.C.c_uint32, _ffi.C.byref
    assert f["traffic_start"](None, 0, 1, 8) == _ffi.EINVAL
    # arguments that can be judged without a meter are SIM_EINVAL before "no meter" is SIM_ESTATE
    buf = np.zeros(4096, np.uint64)
    a, b = u(77), u(78)

    def bad_arguments():
        assert f["traffic_nodes"](g.h, 0, 1, None) == _ffi.EINVAL
        for first, cnt in ((n, 1), (0, n + 1), (n - 1, 2), (0xFFFFFFFF, 2)):
            assert f["traffic_nodes"](g.h, first, cnt, buf.ctypes.data) == _ffi.EINVAL
        for top_k, col in ((0, 0), (65, 0), (8, 8)):
            assert f["traffic_top"](g.h, top_k, col, buf.ctypes.data) == _ffi.EINVAL
        assert f["traffic_top"](g.h, 8, 0, None) == _ffi.EINVAL
        for col, bw in ((8, 1), (0, 0)):
            assert f["traffic_summary"](g.h, col, bw, buf.ctypes.data) == _ffi.EINVAL
        assert f["traffic_summary"](g.h, 0, 1, None) == _ffi.EINVAL
        assert f["traffic_count"](g.h, None, ref(b)) == _ffi.EINVAL and f["traffic_count"](g.h, ref(a), None) == _ffi.EINVAL
        assert f["traffic_count"](None, ref(a), ref(b)) == _ffi.EINVAL
        assert f["traffic_read"](g.h, 0, 0, None, 64, ref(a)) == _ffi.EINVAL and f["traffic_read"](g.h, 0, 0, buf.ctypes.data, 64, None) == _ffi.EINVAL
        assert (a.value, b.value) == (77, 78) and not buf.any()
    bad_arguments()
    m.start(0, 1, 8)
    g.traffic_start(0, 1, 8)
    m.step(3)
    g.step(3)
    same_reads(g, m, "before the errors")
    bad_arguments()                                                        # the same with a meter running
    with pytest.raises(_ffi.SimError) as ei:
        g.traffic_start(0, 0, 8)                                           # bad arguments before "already running"
    assert ei.value.code == _ffi.EINVAL
    with pytest.raises(_ffi.SimError) as ei:
        g.traffic_start(0, 1, 8)
    assert ei.value.code == _ffi.ESTATE
    for first, cnt in ((0, 4), (3, 1), (4, 0)):                           # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.traffic_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL
    small, got = np.zeros(2 * _ffi.TRAFFIC_WORDS, np.uint64), u(77)
    assert f["traffic_read"](g.h, 0, 3, small.ctypes.data, small.size, ref(got)) == _ffi.EINVAL and got.value == 77 and not small.any()
    same_reads(g, m, "after the errors")
    m.step(2)
    g.step(2)
    same_reads(g, m, "two ticks after the errors")
    g.close()
    o.close()
    t = serf_amd.create(256, fanout=3)                                   # inside a tick
    t.traffic_start(0, 1, 8)
    t.step(2)
    t.step_begin()
    for call in every(t):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                                   # a handle destroyed with a meter running
    g.traffic_start(0, 1, 4)
    g.step(6)
    assert g.traffic_count() == (4, 2) and g.traffic_read()["tick"].tolist() == [1, 2, 3, 4]
    g.close()


# ---- 5. restore ----
RESTORE_T = 8


@pytest.mark.parametrize("fan", sorted(tt.FANOUTS))
def test_a_meter_across_a_restore(hiplib, fan):
    """sim_restore takes a fresh handle.  A meter started at tick 0 on a fresh handle that is then restored to tick 8 stays as it
    is: its samples go on behind the ticks t >= 8 — the first of them counts the packets in flight of the image, whose graph
    nobody has built yet — and nothing is counted as dropped.  Then a meter started on a handle that was restored first.  The
    reference: the model on an oracle that restores the same image."""
    n, kw = 1000, tt.churn_kw(1000, fan)
    src = tt.make(n, kw)
    apply_schedule(src, tt.churn_ops(n))
    src.step(RESTORE_T)
    img = src.snapshot()
    for started_first in (True, False):
        o, g = tt.make(n, kw), serf_amd.create(n, **kw)
        m = TrafficModel(o)
        if started_first:
            m.start(0, 1, tt.CHURN_TICKS)
            g.traffic_start(0, 1, tt.CHURN_TICKS)
        o.restore(img)
        g.restore(img)
        assert g.tick == o.tick == RESTORE_T and g.traffic_count() == (0, 0)
        if not started_first:
            m.start(0, 2, tt.CHURN_TICKS)
            g.traffic_start(0, 2, tt.CHURN_TICKS)
        m.step(1)
        g.step(1)
        what = f"a meter {'before' if started_first else 'behind'} a restore, {fan}"
        same_reads(g, m, what + ", the first tick")
        assert g.traffic_read()["tick"].tolist() == [RESTORE_T + 1] and g.traffic_read()["packets"][0] > 0
        m.step(tt.CHURN_TICKS - RESTORE_T - 1)
        g.step(tt.CHURN_TICKS - RESTORE_T - 1)
        same_reads(g, m, what, top_ks=(1, 10, 64))
        assert g.snapshot().tobytes() == o.snapshot().tobytes() and g.digest() == o.digest()
        g.close()
        o.close()
    src.close()
