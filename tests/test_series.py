"""Device-resident time series (include/serf_sim_series.h), the part that needs no GPU: the extension's interface next to
the ABI and the tracker extension it must not disturb, and the reference model (tests/series_model.py) against an
independent route on the oracle (sim_cluster_stats), on a scenario that is asserted to be non-trivial."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_abi
from tests.series_model import SeriesModel, as_records, sample
from tests.test_track import ABI_SYMBOLS_15
from tests.test_track_gpu import BIJECTION, KRANDOM, KW, script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERIES_HEADER = os.path.join(ROOT, "include", "serf_sim_series.h")
TRACK_SYMBOLS_1 = ("track_add", "track_remove", "track_read", "track_active", "track_version")
N, TICKS, QUERY_ID = 4096, 200, 777


HOT_TICK, HOT_BURSTS = 184, (70, 40, 20, 10, 5, 2)


def scenario(n, hot=False):
    """tests/test_track_gpu.py's script (6 crashes, 40 user events of length 64) plus a revive of the first crashed node at
    tick 120, a leave of live[0] at tick 60 and a query with the ACK flag from live[1] at tick 30.
    hot=True adds six hot spots: at tick 184 live[1..5] and the origin of the first user event originate 70 / 40 / 20 / 10 /
    5 / 2 user events each in ONE tick, so that queues of every depth bin — 64 = SIM_Q included, with a few records dropped
    there and counted — stand next to the idle majority; the rumours then flood the cluster, every queue fills up and the
    Q bound drops records everywhere (check_nontrivial says why the plain scenario alone does not get there)."""
    s = script(n)
    acts = [(te, "event", node, key) for te, node, key in s["events"]]
    acts += [(60, "leave", s["live"][0], 0), (30, "query", s["live"][1], QUERY_ID)]
    if hot:
        spots = s["live"][1:6] + [s["events"][0][1]]
        assert len(set(spots)) == len(HOT_BURSTS)
        acts += [(HOT_TICK, "burst", node, cnt) for node, cnt in zip(spots, HOT_BURSTS)]
    s["actions"] = sorted(acts, key=lambda a: a[0])      # (stable: the order of one tick's actions is the list's)
    s["revive"] = (120, s["crashed"][0])
    return s


def drive(sim, s, ticks, step, on_stretch=None):
    """The same script for both sides; the run advances in ONE step(k) per stretch between two injections."""
    for t, c in zip(s["crash_at"], s["crashed"]):
        sim.inject(t, _ffi.OP_CRASH, c)
    sim.inject(s["revive"][0], _ffi.OP_REVIVE, s["revive"][1])
    for t, what, node, arg in s["actions"]:
        if t >= ticks:
            break
        if t > sim.tick:
            step(t - sim.tick)
            if on_stretch:
                on_stretch()
        if what == "event":
            sim.user_event(node, arg, 64)
        elif what == "leave":
            sim.leave(node)
        elif what == "burst":
            for j in range(arg):
                sim.user_event(node, 0x60000000 + (node << 8) + j, 64)
        else:
            sim.query(node, arg, _ffi.F_ACK)
    step(ticks - sim.tick)
    if on_stretch:
        on_stretch()


def variant_kw(variant):
    variant = variant.replace("hot_spots_", "")
    kw = dict(KW, flags=BIJECTION if variant.startswith("bijection") else KRANDOM)
    if variant.endswith("pkt_records_16"):
        kw["pkt_records"] = 16
    if variant == "vshards_4":
        kw["vshards"] = 4
    return kw


def check_nontrivial(o, rec, all_nodes_failed_sum, hot):
    """The scenario does what it is for (otherwise equal samples would show little).  `rec`: the samples of every tick.

    The depth bins.  The plain scenario was meant to show all eight bins in use at one tick (tick 39: [3821, 16, 20, 41, 1,
    26, 120, 46]).  Those figures came from reading SIM_ARR_QUEUE as [slot][node]; the dump is [node][slot] (sim_record
    queue[n][SIM_Q]), which sim_cluster_stats.max_queue confirms at every tick of the test below.  Read the right way the
    plain scenario never holds more than 7 entries in one queue: one user event every 4 ticks, each retransmitted 16 times
    at 4 packets a tick, is one to three events a queue plus the memberlist records of the six crashes — bins 0 .. 3 and no
    further.  So the plain scenario asserts those four bins, and the hot-spot variant (scenario(hot=True)) carries what
    the eight bins were for: all eight in use at ONE tick, queues of SIM_Q entries, the deep-queue path."""
    cs = o.cluster_stats()
    assert cs["ops_dropped"] == 0
    bins = rec["depth_bins"]
    most = bins[(bins > 0).sum(axis=1).argmax()]
    if hot:
        assert (bins > 0).all(axis=1).any(), f"no tick with all eight depth bins in use; most: {most}"
        assert rec["max_depth"].max() == 64 and cs["overflow"] > 0        # SIM_Q entries, and the model bound counted (word 39)
        assert rec["overflow"][HOT_TICK - 1] == 0 and rec["overflow"][HOT_TICK] > 0
    else:
        assert cs["overflow"] == 0                                           # the run stays inside the model's bounds
        assert (bins[:, :4] > 0).all(axis=1).any(), f"no tick with depth bins 0 .. 3 in use; most: {most}"
    assert rec["awareness"][:, 1].max() > 0 and rec["timers"].max() > 0 and rec["nodes_with_timers"].max() > 0
    assert rec["state"][:, 1].max() > 0 and rec["state"][:, 2].max() > 0  # running nodes Leaving (1), then Left (2)
    for k in (_ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY, _ffi.K_SUSPECT, _ffi.K_DEAD):
        assert rec["records"][:, k - 1].max() > 0, f"no record of kind {k} ever in flight"
    assert (rec["clock_max"] > rec["clock_min"]).any()
    assert rec["packets"].max() > 0 and rec["len64"].max() > 0
    # a kernel that forgets the running filter must fail: the sums over running and over all nodes differ at the end
    assert int(rec["n_failed"][-1]) != all_nodes_failed_sum


def series_declared():
    src = re.sub(r"/\*.*?\*/", "", open(SERIES_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t|const char\s*\*)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_series_header_declares_what_the_binding_binds():
    assert series_declared() == sorted("sim_" + s for s in _ffi.SERIES_SYMBOLS)
    assert len(_ffi.SERIES_SYMBOLS) == 5


def test_hip_library_exports_the_series():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in series_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    fn = dll.sim_series_version
    fn.restype = C.c_uint32
    assert fn() == 1
    assert lib.has_series and lib.series_version() == 1


def test_the_abi_and_the_trackers_are_what_they_were(oracle):
    """The series is an extension: serf_sim.h, serf_sim_track.h, ABI_SYMBOLS, TRACK_SYMBOLS and the ABI version do not know
    it; the oracle has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == ABI_SYMBOLS_15
    assert tuple(_ffi.TRACK_SYMBOLS) == TRACK_SYMBOLS_1
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in ABI_SYMBOLS_15)
    assert not set(_ffi.SERIES_SYMBOLS) & (set(_ffi.ABI_SYMBOLS) | set(_ffi.TRACK_SYMBOLS))
    assert serf_amd.load().abi_version() == 15 and oracle.abi_version() == 15
    assert serf_amd.load().track_version() == 1
    assert not oracle.has_series and oracle.series_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.SERIES_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)
    with pytest.raises(NotImplementedError):
        _ffi.Sim(oracle, _ffi.make_config(64)).series_start()


def test_series_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include "serf_sim_series.h"\n'
                    'int main(void){printf("%zu %u %u %u\\n",sizeof(sim_series_sample),SIM_SERIES_WORDS,SIM_SERIES_MAX_SAMPLES,'
                    "SIM_SERIES_VERSION);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [_ffi.SERIES_DTYPE.itemsize, _ffi.SERIES_WORDS, _ffi.SERIES_MAX_SAMPLES, 1]
    assert got[0] == 512
    # the record's fields are the table's words, in order
    off = {n: _ffi.SERIES_DTYPE.fields[n][1] // 8 for n in _ffi.SERIES_DTYPE.names}
    assert off == dict(tick=0, running=1, state=2, queued=6, depth_bins=10, max_depth=18, awareness=19, timers=27,
                       nodes_with_timers=28, n_failed=29, n_left=30, n_known_min=31, n_known_max=32, clock_min=33, clock_max=34,
                       event_clock_min=35, event_clock_max=36, query_clock_min=37, query_clock_max=38, overflow=39, packets=40,
                       records=41, len64=48, reserved=49)


@pytest.mark.parametrize("variant", ["krandomnodes", "bijection_pkt_records_16", "hot_spots_krandomnodes",
                                     "hot_spots_bijection_pkt_records_16"])
def test_model_equals_cluster_stats_at_every_tick(oracle, variant):
    """Two independent routes to the same sums at every tick of the scenario: the model's (dumps + numpy) with
    running_only=False and the oracle's own sim_cluster_stats; then the scenario is asserted to be non-trivial."""
    hot = variant.startswith("hot_spots_")
    s = scenario(N, hot)
    o = _ffi.Sim(oracle, _ffi.make_config(N, **variant_kw(variant)))
    words = []

    def on_tick():
        w, cs = sample(o, running_only=False), o.cluster_stats()
        got = dict(up=int(w[1]), queued=[int(x) for x in w[6:10]], overflow=int(w[39]), failed=int(w[29]), left=int(w[30]),
                   max_queue=int(w[18]), inbox_records=int(w[41:48].sum()))
        assert got == {k: cs[k] for k in got}, f"tick {o.tick}"
        words.append(sample(o))

    m = SeriesModel(o, on_tick)
    drive(o, s, TICKS, m.step)
    rec = as_records(words)
    assert len(rec) == TICKS and rec["tick"].tolist() == list(range(1, TICKS + 1))
    assert (rec["reserved"] == 0).all() and (rec["depth_bins"].sum(axis=1) == rec["running"]).all()
    assert (rec["state"].sum(axis=1) == rec["running"]).all() and (rec["awareness"].sum(axis=1) == rec["running"]).all()
    check_nontrivial(o, rec, int(o.dump(_ffi.ARR_ROWS)["n_failed"].astype(np.int64).sum()), hot)


def test_sampling_rule_of_the_model(oracle):
    o = _ffi.Sim(oracle, _ffi.make_config(256, fanout=3))
    m = SeriesModel(o)
    m.step(4)
    m.start(first_tick=10, period=7, capacity=3)
    m.step(40)
    assert m.count() == (3, 2)                                   # ticks 10, 17, 24 taken; 31, 38 dropped
    assert m.read()[:, 0].tolist() == [11, 18, 25]
    m.stop()
    m.start(first_tick=0, period=2, capacity=100)               # a first tick that has passed: now (44)
    m.step(5)
    assert m.count() == (3, 0) and m.read()[:, 0].tolist() == [45, 47, 49]
