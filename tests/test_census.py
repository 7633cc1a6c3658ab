"""Membership census (include/serf_sim_census.h), the part that needs no GPU: the extension's interface next to the ABI and the
two extensions it must not disturb, and the reference model (tests/census_model.py) against independent routes on the oracle
(sim_members per observer, sim_convergence), on scenarios that are asserted to be non-trivial.

The scenarios (tests/test_census_gpu.py runs the same ones on the GPU) are tests/test_series.scenario — 6 crashes, a revive,
a leave, 40 user events, a query — plus one crash that is revived early (census_drive below), at 4 096 nodes, 200 ticks, a
census behind every tick:

  krandomnodes / bijection / vshards_4   tests/test_track_gpu.KW (loss 0.01, 64 view slots)
  lossy                                  the same with loss LOSSY_LOSS and recycle_interval = 20 (random fan-out)

The lossy variant's loss was picked on the oracle alone (LOSSY_SEEN below has the figures of the losses tried).  Header word 7
(running subjects somebody holds Suspect or Dead) is > 0 in every variant, for the node that is revived at tick 120 runs while
everybody still holds it Dead; what the lossy variant adds is word 7 >= 2: running subjects nobody named beforehand, suspected
because packets were lost.  0.03 is the loss at which that happens (up to 3 at one tick) while the run stays inside its 64 slots
with overflow == 0 and ops_dropped == 0; at 0.05 all 64 slots are taken and the oracle counts dropped operations, at 0.08
sim_leave finds no slot."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_abi
from tests._oracle import load_oracle
from tests.census_model import CensusModel, sample, split, subjects
from tests.test_series import TRACK_SYMBOLS_1, drive, scenario, variant_kw
from tests.test_track import ABI_SYMBOLS_15
from tests.test_track_gpu import KRANDOM, KW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS_HEADER = os.path.join(ROOT, "include", "serf_sim_census.h")
SERIES_SYMBOLS_1 = ("series_start", "series_count", "series_read", "series_stop", "series_version")
N, TICKS, MAX_SUBJECTS = 4096, 200, 64
VARIANTS = ("krandomnodes", "bijection", "vshards_4", "lossy")
LOSSY_LOSS = 0.03
# loss -> (ticks of the 200 with header word 7 > 0, largest word 7, largest word 8, most subjects at one tick, slots recycled,
# overflow, ops_dropped) on the oracle
LOSSY_SEEN = {0.01: (80, 1, 4090, 7, 0, 0, 0), 0.03: (131, 3, 11222, 10, 7, 0, 0), 0.05: (198, 16, 27100, 64, 34, 12, 30)}


def census_kw(variant):
    if variant == "lossy":
        return dict(KW, flags=KRANDOM, loss=LOSSY_LOSS, recycle_interval=20)
    return variant_kw(variant)


EARLY_CRASH, EARLY_REVIVE = 70, 82


def census_drive(sim, s, ticks, step, on_stretch=None):
    """tests/test_series.drive with one more victim: live[2] crashes at tick 70 and is back at tick 82.
    The scenario's own revive (tick 120, 110 ticks after that node's crash) shows a running node everybody holds Failed — for
    good: by then no Suspect or Dead rumour about it travels, so it never hears of its death and never refutes; on the oracle
    every entry's incarnation stays 0 to the end of the run (inc_max == 0 in all 200 samples of all four variants).  A node that
    comes back while the rumours still travel does refute: with this one, incarnation 1 spreads from tick 112 on and
    inc_min < inc_max holds for 88 ticks (63 in the lossy variant) — the min / max words have something to get wrong."""
    sim.inject(EARLY_CRASH, _ffi.OP_CRASH, s["live"][2])
    sim.inject(EARLY_REVIVE, _ffi.OP_REVIVE, s["live"][2])
    drive(sim, s, ticks, step, on_stretch)


@functools.lru_cache(maxsize=None)
def oracle_run(variant, n=N, ticks=TICKS, first=0, period=1, capacity=None, max_subjects=MAX_SUBJECTS, over=()):
    """The scenario on the oracle with the model behind the sampled ticks, once per session: (oracle, model, headers, records).
    Nobody changes what it returns.  over: pairs that override the variant's configuration."""
    o = _ffi.Sim(load_oracle(), _ffi.make_config(n, **dict(census_kw(variant), **dict(over))))
    m = CensusModel(o)
    m.start(first, period, capacity or ticks, max_subjects)
    census_drive(o, scenario(n), ticks, m.step)
    hdr, rec = m.read()
    return o, m, hdr, rec


def check_nontrivial(o, hdr, rec, variant):
    """The scenario does what it is for (otherwise equal samples would show little).  hdr, rec: the samples of every tick."""
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0            # the run stays inside the model's bounds
    assert (hdr["subjects"] <= MAX_SUBJECTS).all() and hdr["subjects"].max() >= 8
    unsettled = np.nonzero(hdr["settled"] < hdr["subjects"])[0]
    agreed = np.nonzero((hdr["settled"] == hdr["subjects"]) & (hdr["subjects"] > 0))[0]
    assert len(unsettled) and len(agreed) and agreed.max() > unsettled.min(), "no disagreement that is settled later"
    assert hdr["stopped_alive"].max() > 0 and hdr["detected"].max() > 0          # the crashes: words 9 and 11
    assert rec["status"][:, :, _ffi.STATUS_LEAVING].max() > 0 and rec["status"][:, :, _ffi.STATUS_LEFT].max() > 0   # the leave
    assert (rec["inc_min"] < rec["inc_max"]).any()                               # the revive: a refutation under way
    assert (rec["ltime_min"] < rec["ltime_max"]).any()
    if variant == "lossy":
        assert hdr["suspected_running"].max() >= 2, "nobody but the revived node was ever suspected while running"   # word 7
        assert cs["slots_recycled"] > 0
    assert hdr["suspected_running"].max() > 0


def census_declared():
    src = re.sub(r"/\*.*?\*/", "", open(CENSUS_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t|const char\s*\*)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_census_header_declares_what_the_binding_binds():
    assert census_declared() == sorted("sim_" + s for s in _ffi.CENSUS_SYMBOLS)
    assert len(_ffi.CENSUS_SYMBOLS) == 6


def test_hip_library_exports_the_census():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in census_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    fn = dll.sim_census_version
    fn.restype = C.c_uint32
    assert fn() == 1
    assert lib.has_census and lib.census_version() == 1


def test_the_abi_the_trackers_and_the_series_are_what_they_were(oracle):
    """The census is an extension: serf_sim.h, serf_sim_track.h, serf_sim_series.h, ABI_SYMBOLS, TRACK_SYMBOLS, SERIES_SYMBOLS
    and the ABI version do not know it; the oracle has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == ABI_SYMBOLS_15
    assert tuple(_ffi.TRACK_SYMBOLS) == TRACK_SYMBOLS_1
    assert tuple(_ffi.SERIES_SYMBOLS) == SERIES_SYMBOLS_1
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in ABI_SYMBOLS_15)
    assert not set(_ffi.CENSUS_SYMBOLS) & (set(_ffi.ABI_SYMBOLS) | set(_ffi.TRACK_SYMBOLS) | set(_ffi.SERIES_SYMBOLS))
    lib = serf_amd.load()
    assert lib.abi_version() == 15 and oracle.abi_version() == 15
    assert lib.track_version() == 1 and lib.series_version() == 1
    assert not oracle.has_census and oracle.census_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.CENSUS_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)
    o = _ffi.Sim(oracle, _ffi.make_config(64))
    for call in (o.census_start, o.census_count, o.census_read, o.census_stop, o.census_now):
        with pytest.raises(NotImplementedError):
            call()


def test_census_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "serf_sim_census.h"\n'
                    'int main(void){printf("%zu %zu %zu %u %u %u\\n",sizeof(sim_census_subject),sizeof(sim_census_header),'
                    "offsetof(sim_census_subject,w[7]),SIM_CENSUS_WORDS,SIM_CENSUS_MAX_SAMPLES,SIM_CENSUS_VERSION);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [_ffi.CENSUS_SUBJECT_DTYPE.itemsize, _ffi.CENSUS_HEADER_DTYPE.itemsize, 56, _ffi.CENSUS_WORDS,
                   _ffi.CENSUS_MAX_SAMPLES, 1]
    assert got[0] == got[1] == 128
    # the records' fields are the tables' words, in order
    off = {n: _ffi.CENSUS_SUBJECT_DTYPE.fields[n][1] // 8 for n in _ffi.CENSUS_SUBJECT_DTYPE.names}
    assert off == dict(id=0, running=1, status=2, swim=7, intents=11, ltime_min=12, ltime_max=13, inc_min=14, inc_max=15)
    off = {n: _ffi.CENSUS_HEADER_DTYPE.fields[n][1] // 8 for n in _ffi.CENSUS_HEADER_DTYPE.names}
    assert off == dict(tick=0, running=1, subjects=2, stored=3, settled=4, false_failed=5, false_failed_pairs=6,
                       suspected_running=7, suspected_running_pairs=8, stopped_alive=9, stopped_alive_pairs=10, detected=11,
                       reserved=12)


def test_sampling_rule_of_the_model(oracle):
    o = _ffi.Sim(oracle, _ffi.make_config(256, fanout=3))
    m = CensusModel(o)
    m.step(4)
    m.start(first_tick=10, period=7, capacity=3, max_subjects=5)
    m.step(40)
    assert m.count() == (3, 2)                                   # ticks 10, 17, 24 taken; 31, 38 dropped
    hdr, rec = m.read()
    assert hdr["tick"].tolist() == [11, 18, 25] and rec.shape == (3, 5)
    assert (hdr["subjects"] == 256).all() and (hdr["stored"] == 5).all() and (hdr["settled"] == 256).all()
    m.stop()
    m.start(first_tick=0, period=2, capacity=100)               # a first tick that has passed: now (44)
    m.step(5)
    assert m.count() == (3, 0) and m.read()[0]["tick"].tolist() == [45, 47, 49]
    h, r = m.now(3)
    assert int(h["tick"]) == 49 and int(h["stored"]) == 3 and len(r) == 3 and int(h["subjects"]) == 256


def test_model_equals_members_and_convergence_at_256_nodes(oracle):
    """Two independent routes on the oracle: sim_members(observer) for every running observer rebuilds words 2-6, 12 and 13
    of every subject; sim_convergence(JOIN / LEAVE, subject, ltime) — running nodes that know the subject at that Lamport time
    or later — rebuilds the known count and brackets the two extremes."""
    n = 256
    o = _ffi.Sim(oracle, _ffi.make_config(n, fanout=3, view_slots=32, probe_interval=5, loss=0.02, push_pull_interval=150,
                                          join_sync=True, event_ring=64, query_ring=64))
    for t, c in ((3, 17), (6, 200), (9, 90)):
        o.inject(t, _ffi.OP_CRASH, c)
    o.inject(60, _ffi.OP_REVIVE, 17)
    seen_disagreement = False
    for stretch, act in ((12, lambda: o.leave(5)), (30, lambda: None), (40, lambda: o.join(5, 7)), (30, lambda: None)):
        o.step(stretch)
        act()
        words = sample(o, 32)
        hdr, rec = split(words, 32)
        hdr, rec = hdr[0], rec[0][:int(hdr[0]["stored"])]
        slots, subj = subjects(o)
        assert (rec["id"] & 0xFFFFFFFF).tolist() == subj.tolist() and (rec["id"] >> 32).tolist() == slots.tolist()
        rows = o.dump(_ffi.ARR_ROWS)
        up = np.nonzero(rows["flags"] & 1)[0]
        assert int(hdr["running"]) == len(up) and len(subj) >= 4
        st_all, lt_all = zip(*(o.members(int(obs)) for obs in up))
        st_all, lt_all = np.array(st_all), np.array(lt_all)                     # [observer][subject]
        for r, x in zip(rec, subj.tolist()):
            st, lt = st_all[:, x], lt_all[:, x]
            assert [int((st == b).sum()) for b in range(5)] == r["status"].tolist(), f"subject {x}"
            known = st != _ffi.STATUS_NONE
            want = (int(lt[known].min()), int(lt[known].max())) if known.any() else (0, 0)
            assert (int(r["ltime_min"]), int(r["ltime_max"])) == want, f"subject {x}"
            nknown = len(up) - int(r["status"][0])
            for kind in (_ffi.K_JOIN, _ffi.K_LEAVE):
                assert o.convergence(kind, x, 0) == (nknown, len(up))
                if nknown:
                    assert o.convergence(kind, x, int(r["ltime_min"])) == (nknown, len(up))
                    assert o.convergence(kind, x, int(r["ltime_max"]))[0] >= 1
                    assert o.convergence(kind, x, int(r["ltime_max"]) + 1)[0] == 0
                    if r["ltime_min"] < r["ltime_max"]:
                        assert o.convergence(kind, x, int(r["ltime_min"]) + 1)[0] < nknown
                        seen_disagreement = True
            assert int(r["running"]) == int(rows["flags"][x] & 1)
    assert seen_disagreement
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_scenarios_are_nontrivial_on_the_oracle(variant):
    o, m, hdr, rec = oracle_run(variant)
    assert m.count() == (TICKS, 0) and hdr["tick"].tolist() == list(range(1, TICKS + 1))
    assert (hdr["reserved"] == 0).all()
    stored = hdr["stored"].astype(np.int64)
    assert (stored == np.minimum(hdr["subjects"], MAX_SUBJECTS)).all()
    for i in (0, TICKS // 2, TICKS - 1):                               # the bins' sums, and zeros beyond what is stored
        r = rec[i][:stored[i]]
        assert (r["status"].sum(axis=1) == hdr["running"][i]).all()
        assert (r["swim"].sum(axis=1) == hdr["running"][i] - r["status"][:, 0]).all()
        assert not rec[i][stored[i]:].view(np.uint64).any()
        assert (np.diff((r["id"] >> 32).astype(np.int64)) > 0).all()   # ascending slot order
    check_nontrivial(o, hdr, rec, variant)
