"""The traffic meter's reference model (tests/traffic_model.py) against routes that do not share its code, on the CPU oracle: the
series' and the ledger's totals of the packets in flight, the conservation of packets between senders and targets, the spread
map's arrivals in a cluster where one event is all that travels; the vectorised target draw against
tests/third_model.py::k_random_nodes; the sampling rules; the symbols the HIP library exports.  This file owns the scenarios
tests/test_traffic_gpu.py drives the HIP library through.  Everything compared is an exact integer."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from serf_amd.workload import apply_schedule, schedule
from tests import ledger_model, series_model
from tests._oracle import load_oracle
from tests.spread_model import SpreadModel
from tests.third_model import k_random_nodes
from tests.traffic_model import TrafficModel, k_random_nodes_all

KRANDOM = _ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT
BIJECTION = _ffi.CF_BASELINE_JOINED
FANOUTS = {"krandomnodes": KRANDOM, "bijection": BIJECTION}
FANOUT = 4
CHURN_TICKS = 20
TRAFFIC_GRID = 1024                       # serf_sim_traffic.inc: #define TRAFFIC_GRID 1024u; per_pass = gridDim.x * BLOCK
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "serf_amd", "csrc")
CHURN_MIX = (0.4, 0.1, 0.1, 0.2, 0.2)          # user event, query, leave, crash + force-leave, crash + revive


def churn_kw(n, fan, **more):
    """No SWIM layer unless asked for: nobody notices a crash, the stopped processes keep being addressed."""
    return dict(dict(fanout=FANOUT, view_slots=0 if n <= 65 else 32, event_ring=64, query_ring=64, ring_overflow=4, flags=FANOUTS[fan]), **more)


def churn_ops(n, ticks=CHURN_TICKS, burst=0):
    """A small churn schedule, every operation injected up front: about two operations a tick, crashes among them from the first
    ticks on; burst: that many small user events in ticks 0 .. 7 on top (with PKT16: enough queued records to fill a 16-record packet)."""
    ops = schedule(n, max(4, ticks - 6), 2.0, seed=1000 + n, mix=CHURN_MIX, max_member_subjects=min(n // 3, 8))
    ops = [o for o in ops if o[2] < n and o[0] < ticks]
    if n >= 4:
        ops += [(1, _ffi.OP_CRASH, n - 1, 0, 0), (3, _ffi.OP_CRASH, n // 2, 0, 0), (9, _ffi.OP_REVIVE, n // 2, 0, 0)]
    ops += [(i % 8, _ffi.OP_USER_EVENT, (7 * i) % n, 5000 + i, 16) for i in range(burst)]
    return sorted(ops, key=lambda o: o[0])


def make(n, kw):
    return _ffi.Sim(load_oracle(), _ffi.make_config(n, **kw))


def model_run(n, kw, ops, ticks, each=None, **start):
    """The schedule on a fresh oracle with the model started at tick 0 and stepped tick by tick; each(o, m) behind every tick.
    Returns (oracle, model)."""
    o = make(n, kw)
    m = TrafficModel(o, (lambda: each(o, m)) if each else None)
    m.start(**dict(dict(first_tick=0, period=1, capacity=ticks), **start))
    apply_schedule(o, ops)
    m.step(ticks)
    return o, m


# ---- the target draw ----
@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 6, 64, 257))
def test_the_vectorised_draw_is_k_random_nodes(n):
    for seed, tick in ((_ffi.DEFAULT_SEED, 0), (_ffi.DEFAULT_SEED, 7), (12345, 123456789)):
        for fanout in (1, 3, 4):
            got = k_random_nodes_all(seed, tick, n, fanout)
            for node in range(n):
                want = k_random_nodes(seed, tick, node, n, fanout)
                assert got[node][:len(want)].tolist() == want and (got[node][len(want):] == -1).all(), (n, seed, tick, fanout, node)


# ---- 1. totals, 2. conservation ----
# records that stay queued for 12 x 3 transmits: with a burst of 16 events a node
# queues 16 records and more, and the run stays inside the model's bounds
PKT16 = dict(pkt_records=16, retransmit_mult=12)
PKT16_BURST = 16
VARIANTS = {"loss": dict(loss=0.3), "pkt16": PKT16, "loss+pkt16": dict(PKT16, loss=0.3)}
TOTALS_N, TOTALS_TICKS = 257, 24
DUMMY_ENTRY = [(_ffi.K_EVENT, 1, 1)]


@functools.lru_cache(maxsize=None)
def totals_run(fan, variant):
    """Per tick: the model's sample and map, series_model's and ledger_model's words of the same state."""
    kw = churn_kw(TOTALS_N, fan, **VARIANTS[variant])
    series, ledger, maps = [], [], []

    def each(o, m):
        series.append(series_model.sample(o))
        ledger.append(ledger_model.sample(o, DUMMY_ENTRY))
        maps.append(m.map.copy())
    o, m = model_run(TOTALS_N, kw, churn_ops(TOTALS_N, TOTALS_TICKS, burst=PKT16_BURST if "pkt16" in variant else 0), TOTALS_TICKS, each)
    return dict(o=o, m=m, samples=m.read(), series=series, ledger=ledger, maps=maps)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("fan", sorted(FANOUTS))
def test_totals_are_the_series_and_the_ledgers(fan, variant):
    run = totals_run(fan, variant)
    s = run["samples"]
    assert len(s) == TOTALS_TICKS and s["tick"].tolist() == list(range(1, TOTALS_TICKS + 1))
    for i in range(TOTALS_TICKS):
        ser, led = run["series"][i], run["ledger"][i]
        assert (s["packets"][i], s["records"][i], s["units"][i]) == (ser[40], ser[41:48].sum(), ser[48]), f"tick {i}: the series"
        assert (s["packets"][i], s["records"][i]) == (led[5], led[4]), f"tick {i}: the ledger"
        assert s["running"][i] == ser[1]
    # the scenario moves what it is for
    assert s["packets"].max() > TOTALS_N and s["running"].min() < TOTALS_N and s["to_down"].sum() > 0
    cs = run["o"].cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0            # the run stays inside the model's bounds
    if "pkt16" in variant:
        assert s["packet_records_max"].max() == 16, "a packet of four full pages: the 5-bit records field at its largest"
        assert s["packet_units_max"].max() == 87, "a packet at the byte budget: the 7-bit units field at its largest"
    if "loss" in variant:
        assert (s["packets"] < s["senders"] * FANOUT).any(), "loss removed packets of nodes that sent others"


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("fan", sorted(FANOUTS))
def test_conservation(fan, variant):
    run = totals_run(fan, variant)
    s = run["samples"]
    prev = np.zeros_like(run["maps"][0]).astype(np.int64)
    peak = np.zeros(TOTALS_N, np.int64)
    for i, cum in enumerate(run["maps"]):
        cum = cum.astype(np.int64)
        d = cum - prev
        prev = cum
        for tx, rx in ((0, 3), (1, 4), (2, 5)):
            assert cum[tx].sum() == cum[rx].sum() and d[tx].sum() == d[rx].sum(), f"sample {i}: columns {tx} / {rx}"
        assert (d[0].sum(), d[1].sum(), d[2].sum()) == (s["packets"][i], s["records"][i], s["units"][i])
        assert s["degree_bins"][i].sum() == TOTALS_N and s["record_bins"][i].sum() == s["packets"][i]
        assert (s["record_bins"][i] * np.arange(1, 17)).sum() == s["records"][i]
        assert d[7].sum() == s["to_down"][i] and (d[3] > 0).sum() == s["addressed"][i] and (d[0] > 0).sum() == s["senders"][i]
        assert s["max_packets"][i] == d[3].max() and s["max_units"][i] == d[5].max()
        if fan == "bijection":
            assert d[3].max() <= FANOUT and not s["degree_bins"][i][FANOUT + 1:].any(), "nobody is addressed by more than feff packets"
        peak = np.maximum(peak, d[3])
        assert (cum[6] == peak).all(), f"sample {i}: rx_peak"
    if fan == "krandomnodes":
        assert s["max_packets"].max() > FANOUT, "Poisson-like in-degree: somebody is addressed by more than fanout packets"


# ---- 3. the spread map ----
SPREAD_N, SPREAD_TICKS, SPREAD_ORIGIN, SPREAD_KEY = 257, 25, 5, 0x77


@pytest.mark.parametrize("fan", sorted(FANOUTS))
def test_first_addressed_is_the_spread_maps_arrival(fan):
    """One user event into an otherwise idle cluster is the only record that travels: a packet in flight behind tick t is applied
    during tick t + 1 and the spread map latches that at now = t + 2 = 1 + the sample's now."""
    kw = dict(fanout=FANOUT, view_slots=16, event_ring=64, query_ring=64, flags=FANOUTS[fan])
    o = make(SPREAD_N, kw)
    entry = (_ffi.K_EVENT, SPREAD_KEY, o.stats(SPREAD_ORIGIN).event_time)
    first = np.zeros(SPREAD_N, np.int64)
    tm = TrafficModel(o)

    def each():
        before = tm.map[3].astype(np.int64)
        tm.after_tick(o.tick - 1)
        hit = (tm.map[3].astype(np.int64) > before) & (first == 0)
        first[hit] = o.tick
    sm = SpreadModel(o, each)
    sm.start([entry], 0, 1, SPREAD_TICKS)
    tm.start(0, 1, SPREAD_TICKS)
    o.user_event(SPREAD_ORIGIN, SPREAD_KEY, 64)
    sm.step(SPREAD_TICKS)
    arrival = sm.map(0).astype(np.int64)
    others = np.arange(SPREAD_N) != SPREAD_ORIGIN
    assert arrival[SPREAD_ORIGIN] == 1 and (arrival[others] > 0).sum() > SPREAD_N // 2
    want = np.where(first > 0, first + 1, 0)
    late = first == SPREAD_TICKS                      # addressed behind the last tick: applied during a tick that did not run
    assert (arrival[others & ~late] == want[others & ~late]).all() and (arrival[others & late] == 0).all()
    assert tm.read()["records"].tolist() == tm.read()["packets"].tolist(), "one record a packet: the event alone"
    o.close()


# ---- the sampling rules (what tests/test_traffic_gpu.py expects of the library) ----
def test_period_first_tick_full_buffer_and_restart():
    n, kw = 65, churn_kw(65, "krandomnodes")
    o, m = model_run(n, kw, churn_ops(n), CHURN_TICKS, first_tick=5, period=3, capacity=4)
    s = m.read()
    assert s["tick"].tolist() == [6, 9, 12, 15] and m.count() == (4, 1) and s["samples"].tolist() == [1, 2, 3, 4]
    assert m.summary(0)["samples"] == 4 and m.nodes()["tx_packets"].sum() == s["packets"].sum(), "the dropped sample added nothing"
    m.stop()
    m.start(0, 1, 8)
    assert not m.map.any() and m.count() == (0, 0)
    m.step(2)
    assert m.read()["tick"].tolist() == [CHURN_TICKS + 1, CHURN_TICKS + 2] and m.read()["samples"].tolist() == [1, 2]
    top = m.top(64, 3)
    assert top["id"][:n].tolist() == np.lexsort((np.arange(n), -m.nodes()["rx_packets"].astype(np.int64))).tolist()[:64]
    o.close()


def test_rates():
    nodes = np.zeros(4, _ffi.TRAFFIC_NODE_DTYPE)
    nodes["tx_units"], nodes["rx_units"] = [10, 20, 30, 40], [0, 0, 0, 100]
    r = _ffi.traffic_rates(nodes, samples=5, interval_ms=200)       # one second
    assert r["tx"].tolist() == [160.0, 320.0, 480.0, 640.0] and r["rx_stats"]["max"] == 1600.0 and r["tx_stats"]["median"] == 400.0
    assert r["rx_stats"]["median"] == 0.0 and 0.0 < r["rx_stats"]["p99"] <= 1600.0


def test_the_cap_is_the_sources():
    """TRAFFIC_GRID mirrors the source; a change there has to move the second-pass size of tests/test_traffic_gpu.py."""
    src = open(os.path.join(CSRC, "serf_sim_traffic.inc")).read()
    assert re.search(r"^#define TRAFFIC_GRID 1024u\b", src, re.M) and src.count("const size_t per_pass = (size_t)gridDim.x * BLOCK;") == 2
    assert "for (size_t l = (size_t)blockIdx.x * BLOCK + threadIdx.x; l < Nl; l += (size_t)gridDim.x * BLOCK)" in src


# ---- 4. exports ----
def test_exports_without_a_device():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    assert len(_ffi.TRAFFIC_SYMBOLS) == 8
    for name in _ffi.TRAFFIC_SYMBOLS:
        assert hasattr(dll, "sim_" + name), name
    assert lib.has_traffic and lib.traffic_version() == 1
    dll.sim_traffic_version.restype = C.c_uint32
    assert dll.sim_traffic_version() == 1
    assert C.sizeof(_ffi.TrafficNode) == 32 and C.sizeof(_ffi.TrafficRank) == 40
    assert _ffi.TRAFFIC_NODE_DTYPE.itemsize == 32 and _ffi.TRAFFIC_RANK_DTYPE.itemsize == 40
