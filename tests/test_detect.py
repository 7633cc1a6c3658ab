"""Detection log (include/serf_sim_detect.h), the part that needs no GPU: the extension's interface next to the ABI and the five
extensions it must not disturb, and the reference model (tests/detect_model.py: a fold over the census records of
tests/census_model.py) on the oracle — on the census's scenarios (tests/test_census.census_drive), asserted to be as rich as a
prototype of the rules found them, against an independent route (MEMBER trackers of tests/track_model.py registered for the
scheduled crashes) and on a crash injected into an accusation.

The scenario, 4 096 nodes x 200 ticks, a sample behind every tick: six crashes at ticks 10, 17 .. 45 (the first is revived at
tick 120, after everybody declared it failed: it never hears of it and stays accused), live[2] crashes at tick 70 and is back at
82 (RETURNED, then accused AFTER_RETURN until its refutation has spread: CLEARED), live[0] leaves at tick 60 (its DOWN episode
is still open at the end).  The lossy variant adds running nodes that are suspected because packets were lost, and cleared."""
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
from tests.detect_model import DetectModel
from tests.test_census import EARLY_CRASH, EARLY_REVIVE, SERIES_SYMBOLS_1, census_drive, census_kw
from tests.test_ledger import ROLL_SYMBOLS_1
from tests.test_roll import CENSUS_SYMBOLS_1
from tests.test_series import TRACK_SYMBOLS_1, scenario
from tests.test_track import ABI_SYMBOLS_15
from tests.track_model import TrackModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETECT_HEADER = os.path.join(ROOT, "include", "serf_sim_detect.h")
LEDGER_SYMBOLS_1 = ("ledger_start", "ledger_count", "ledger_read", "ledger_stop", "ledger_now", "ledger_version")
N, TICKS = 4096, 200
NEVER = _ffi.DETECT_NEVER
FAILED_OR_LEFT = 1 << _ffi.STATUS_FAILED | 1 << _ffi.STATUS_LEFT
SUSPECT_OR_DEAD = 1 << _ffi.SWIM_SUSPECT | 1 << _ffi.SWIM_DEAD
# (DETECTED, RETURNED, CLEARED) a prototype of the rules found on this tree's oracle: the run is to be at least this rich
RICH = {"krandomnodes": (6, 1, 1), "lossy": (6, 1, 10)}


def drive_with(o, m, n, ticks, extra=()):
    """census_drive with the model behind every tick; extra: (tick, op, node) injected up front."""
    for t, op, node in extra:
        o.inject(t, op, node)
    census_drive(o, scenario(n), ticks, m.step)


@functools.lru_cache(maxsize=None)
def oracle_run(variant, n=N, ticks=TICKS, first=0, period=1, capacity=None, log_capacity=1 << 16, over=(), extra=()):
    """The scenario on the oracle with the model behind the sampled ticks, once per session: (oracle, model, headers, log,
    open episodes).  Nobody changes what it returns."""
    o = _ffi.Sim(load_oracle(), _ffi.make_config(n, **dict(census_kw(variant), **dict(over))))
    m = DetectModel(o)
    if first <= 0:
        m.start(first, period, capacity or ticks, log_capacity)
        drive_with(o, m, n, ticks, extra)
    else:                                   # a log that starts when the run has reached tick `first`
        started = []

        def step(k):
            for _ in range(k):
                if o.tick == first and not started:
                    m.start(first, period, capacity or ticks, log_capacity)
                    started.append(1)
                m.step(1)
        for t, op, node in extra:
            o.inject(t, op, node)
        census_drive(o, scenario(n), ticks, step)
    return o, m, m.read(), m.log(), m.open()


def by_outcome(log):
    return [int(((log["outcome"] == oc)).sum()) for oc in range(1, 6)]


def check_consistent(hdr, log, opened, lost=0):
    """What a log's three parts say about each other (model or library).  log: every record, nothing lost — or `lost` of them."""
    last = hdr[-1]
    assert int(last["log_written"]) == len(log) and int(last["log_lost"]) == lost
    assert int(hdr["closed_now"].sum()) == len(log) + lost == int(last["closed"].sum())
    assert (np.diff(hdr["log_written"].astype(np.int64) + hdr["log_lost"].astype(np.int64)) == hdr["closed_now"][1:]).all()
    assert int(last["open_down"]) == int((opened["kind"] == _ffi.DETECT_DOWN).sum())
    assert int(last["open_accused"]) == int((opened["kind"] == _ffi.DETECT_ACCUSED).sum())
    assert int(last["open_down"]) + int(last["open_accused"]) == len(opened)
    assert (opened["closed"] == NEVER).all() and (opened["outcome"] == 0).all() and (np.diff(opened["slot"].astype(np.int64)) > 0).all()
    if not lost:
        assert by_outcome(log) == last["closed"].tolist()
        assert int(last["false_declared"]) == int(((log["kind"] == _ffi.DETECT_ACCUSED) & (log["first_failed"] != NEVER)).sum())
        assert int(last["opened_down"]) == int((log["kind"] == _ffi.DETECT_DOWN).sum()) + int(last["open_down"])
        assert int(last["opened_accused"]) == int((log["kind"] == _ffi.DETECT_ACCUSED).sum()) + int(last["open_accused"])
        det = log[(log["outcome"] == _ffi.DETECT_DETECTED) & ((log["flags"] & _ffi.DETECT_F_CENSORED) == 0)]
        clr = log[log["outcome"] == _ffi.DETECT_CLEARED]
        assert int(last["hist_suspect"].sum()) == int(last["hist_all"].sum()) == len(det) and int(last["hist_cleared"].sum()) == len(clr)
        for field, x in (("hist_all", det["all"] - det["opened"]), ("hist_cleared", clr["closed"] - clr["opened"])):
            want = np.bincount([_ffi.detect_bin(int(v)) for v in x], minlength=16)
            assert last[field].tolist() == want.tolist(), field
        want = np.bincount([15 if int(e["first_suspect"]) == NEVER else _ffi.detect_bin(int(e["first_suspect"]) - int(e["opened"])) for e in det],
                           minlength=16)
        assert last["hist_suspect"].tolist() == want.tolist()
    for e in list(log) + list(opened):                                # an episode's own words
        assert int(e["zero"]) == 0 and int(e["kind"]) in (1, 2) and int(e["evaluated"]) >= 1
        if e["kind"] == _ffi.DETECT_ACCUSED:
            assert e["first_suspect"] == e["opened"] and e["half"] == e["p99"] == e["all"] == NEVER
        if e["outcome"] == _ffi.DETECT_DETECTED:
            assert e["kind"] == _ffi.DETECT_DOWN and e["all"] == e["closed"] and e["opened"] <= e["half"] <= e["p99"] <= e["all"]


def detect_declared():
    src = re.sub(r"/\*.*?\*/", "", open(DETECT_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t|const char\s*\*)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_detect_header_declares_what_the_binding_binds():
    assert detect_declared() == sorted("sim_" + s for s in _ffi.DETECT_SYMBOLS)
    assert len(_ffi.DETECT_SYMBOLS) == 8


def test_hip_library_exports_the_detection_log():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in detect_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    fn = dll.sim_detect_version
    fn.restype = C.c_uint32
    assert fn() == 1
    assert lib.has_detect and lib.detect_version() == 1


def test_the_abi_and_the_five_older_extensions_are_what_they_were(oracle):
    """The detection log is an extension: serf_sim.h, the five older extensions' headers and symbol lists and the ABI version
    do not know it; the oracle has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == ABI_SYMBOLS_15
    assert tuple(_ffi.TRACK_SYMBOLS) == TRACK_SYMBOLS_1
    assert tuple(_ffi.SERIES_SYMBOLS) == SERIES_SYMBOLS_1
    assert tuple(_ffi.CENSUS_SYMBOLS) == CENSUS_SYMBOLS_1
    assert tuple(_ffi.ROLL_SYMBOLS) == ROLL_SYMBOLS_1
    assert tuple(_ffi.LEDGER_SYMBOLS) == LEDGER_SYMBOLS_1
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in ABI_SYMBOLS_15)
    older = set(_ffi.ABI_SYMBOLS) | set(_ffi.TRACK_SYMBOLS) | set(_ffi.SERIES_SYMBOLS) | set(_ffi.CENSUS_SYMBOLS) | set(_ffi.ROLL_SYMBOLS) | set(_ffi.LEDGER_SYMBOLS)
    assert not set(_ffi.DETECT_SYMBOLS) & older
    lib = serf_amd.load()
    assert lib.abi_version() == 15 and oracle.abi_version() == 15
    assert (lib.track_version(), lib.series_version(), lib.census_version(), lib.roll_version(), lib.ledger_version()) == (1, 1, 1, 1, 1)
    assert not oracle.has_detect and oracle.detect_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.DETECT_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)
    o = _ffi.Sim(oracle, _ffi.make_config(64))
    for call in (o.detect_start, o.detect_count, o.detect_read, o.detect_log_count, o.detect_log, o.detect_open, o.detect_stop):
        with pytest.raises(NotImplementedError):
            call()


def test_detect_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "serf_sim_detect.h"\n'
                    'int main(void){printf("%zu %zu %u %u %u %u %u %u %d %d %d %d %d\\n",sizeof(sim_detect_episode),sizeof(sim_detect_header),'
                    "SIM_DETECT_WORDS,SIM_DETECT_EPISODE_WORDS,SIM_DETECT_MAX_SAMPLES,SIM_DETECT_MAX_LOG,SIM_DETECT_NEVER,SIM_DETECT_VERSION,"
                    "SIM_DETECT_DOWN,SIM_DETECT_ACCUSED,SIM_DETECT_DETECTED,SIM_DETECT_ABANDONED,SIM_DETECT_F_AFTER_RETURN);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [_ffi.DETECT_EPISODE_DTYPE.itemsize, _ffi.DETECT_HEADER_DTYPE.itemsize, _ffi.DETECT_WORDS, _ffi.DETECT_EPISODE_WORDS,
                   _ffi.DETECT_MAX_SAMPLES, _ffi.DETECT_MAX_LOG, _ffi.DETECT_NEVER, 1, _ffi.DETECT_DOWN, _ffi.DETECT_ACCUSED,
                   _ffi.DETECT_DETECTED, _ffi.DETECT_ABANDONED, _ffi.DETECT_F_AFTER_RETURN]
    assert got[:6] == [64, 512, 64, 8, 1 << 20, 1 << 24]
    # the records' fields are the tables' words and their halves, in order (byte offsets for the episode)
    off = {n: _ffi.DETECT_HEADER_DTYPE.fields[n][1] // 8 for n in _ffi.DETECT_HEADER_DTYPE.names}
    assert off == dict(tick=0, running=1, subjects=2, open_down=3, open_accused=4, closed_now=5, log_written=6, log_lost=7, closed=8,
                       false_declared=13, opened_down=14, opened_accused=15, hist_suspect=16, hist_all=32, hist_cleared=48)
    off = {n: _ffi.DETECT_EPISODE_DTYPE.fields[n][1] for n in _ffi.DETECT_EPISODE_DTYPE.names}
    assert off == dict(subject=0, slot=4, kind=8, outcome=9, flags=10, zero=12, opened=16, closed=20, first_suspect=24, first_failed=28,
                       half=32, p99=36, all=40, evaluated=44, peak=48, peak_susp=56)
    assert [_ffi.detect_bin(x) for x in (0, 1, 2, 3, 4, 7, 8, 16383, 16384, 1 << 31)] == [0, 1, 2, 2, 3, 3, 4, 14, 15, 15]


def test_sampling_rule_of_the_model(oracle):
    o = _ffi.Sim(oracle, _ffi.make_config(256, fanout=3))
    m = DetectModel(o)
    m.step(4)
    m.start(first_tick=10, period=7, capacity=3, log_capacity=5)
    m.step(40)
    assert m.count() == (3, 2)                                   # ticks 10, 17, 24 taken; 31, 38 dropped
    hdr = m.read()
    assert hdr["tick"].tolist() == [11, 18, 25] and (hdr["subjects"] == 256).all() and (hdr["running"] == 256).all()
    assert m.log_count() == (0, 0) and len(m.log()) == 0 and len(m.open()) == 0 and not hdr.view(np.uint64).reshape(3, 64)[:, 3:].any()
    m.stop()
    m.start(first_tick=0, period=2, capacity=100)               # a first tick that has passed: now (44)
    m.step(5)
    assert m.count() == (3, 0) and m.read()["tick"].tolist() == [45, 47, 49]
    assert len(m.read(1, 1)) == 1 and int(m.read(1, 1)["tick"][0]) == 47


@pytest.mark.parametrize("variant", sorted(RICH))
def test_the_scenario_does_what_it_is_for(variant):
    o, m, hdr, log, opened = oracle_run(variant)
    s = scenario(N)
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    assert m.count() == (TICKS, 0) and hdr["tick"].tolist() == list(range(1, TICKS + 1))
    got = by_outcome(log)
    print(variant, "closed by outcome", got, "open", [(int(e["kind"]), int(e["subject"])) for e in opened])
    assert hdr["closed"][-1].tolist() == got and m.log_count() == (len(log), 0)
    want = RICH[variant]
    assert got[0] >= want[0] and got[1] >= want[1] and got[2] >= want[2], f"{got} is poorer than {want}"
    det = log[log["outcome"] == _ffi.DETECT_DETECTED]
    assert sorted(det["subject"].tolist()) == sorted(s["crashed"])                     # every scheduled crash, nobody else
    assert (det["opened"] == np.array([t + 1 for t in s["crash_at"]])[np.argsort(np.argsort(det["opened"]))]).all()
    ret = log[log["outcome"] == _ffi.DETECT_RETURNED]
    assert ret["subject"].tolist() == [s["live"][2]] and ret["opened"].tolist() == [EARLY_CRASH + 1] and ret["closed"].tolist() == [EARLY_REVIVE + 1]
    after = log[(log["flags"] & _ffi.DETECT_F_AFTER_RETURN) != 0]
    assert after["subject"].tolist() == [s["live"][2]] and after["outcome"].tolist() == [_ffi.DETECT_CLEARED] and after["opened"].tolist() == [EARLY_REVIVE + 1]
    if variant == "krandomnodes":
        assert ((det["first_suspect"] - det["opened"]) <= 4).all() and (det["first_suspect"] >= det["opened"]).all()
        lat = (det["all"] - det["opened"]).astype(np.int64)
        assert lat.min() >= 72 and lat.max() <= 83
        assert [(int(e["kind"]), int(e["subject"])) for e in opened if e["kind"] == _ffi.DETECT_ACCUSED] == [(_ffi.DETECT_ACCUSED, s["revive"][1])]
        assert int((opened["kind"] == _ffi.DETECT_DOWN).sum()) >= 1 and s["live"][0] in opened["subject"].tolist()
        acc = opened[opened["kind"] == _ffi.DETECT_ACCUSED][0]
        assert int(acc["opened"]) == s["revive"][0] + 1 and int(acc["first_failed"]) == s["revive"][0] + 1 and int(acc["flags"]) == 0
    else:
        assert hdr["closed_now"].max() >= 2, "no sample closes two episodes"
        assert cs["slots_recycled"] > 0
    assert not (log["flags"] & _ffi.DETECT_F_CENSORED).any()
    check_consistent(hdr, log, opened)
    summ = _ffi.detect_summary(np.concatenate([log, opened]))
    assert summ["down/detected"]["count"] == got[0] and summ["down/detected"]["all"]["n"] == got[0]
    assert summ["down/detected"]["all"]["median"] == float(np.median((det["all"] - det["opened"]).astype(np.int64)))
    assert summ["accused/cleared"]["count"] == got[2] and summ["accused/open"]["count"] == int((opened["kind"] == 2).sum())


def test_trackers_latch_what_the_down_episodes_latch(oracle):
    """The independent route: for each scheduled crash (and the early one, which returns) two MEMBER trackers on the oracle,
    started at the crash tick — "Failed or Left" and "suspected or worse" — latch the ticks the DOWN episode holds."""
    s = scenario(N)
    o = _ffi.Sim(oracle, _ffi.make_config(N, **census_kw("krandomnodes")))
    tm = TrackModel(o)
    m = DetectModel(o, on_tick=tm.evaluate)
    m.start(0, 1, TICKS, 1 << 10)
    crashes = list(zip(s["crash_at"], s["crashed"], [0] * 6)) + [(EARLY_CRASH, s["live"][2], EARLY_REVIVE - EARLY_CRASH)]
    ids = [(c, tm.add(_ffi.member_tracker(c, FAILED_OR_LEFT, start=t, max_age=age)),
            tm.add(_ffi.member_tracker(c, 1 << _ffi.STATUS_FAILED, SUSPECT_OR_DEAD, start=t, max_age=age))) for t, c, age in crashes]
    census_drive(o, s, TICKS, m.step)
    down = {int(e["subject"]): e for e in m.log() if e["kind"] == _ffi.DETECT_DOWN}
    assert sorted(down) == sorted(c for _, c, _ in crashes)
    for c, gone, worse in ids:
        e, g, w = down[c], tm.result(gone), tm.result(worse)
        assert (int(e["first_failed"]), int(e["half"]), int(e["p99"]), int(e["all"])) == (g["first"], g["half"], g["p99"], g["all"]), f"subject {c}"
        assert int(e["first_suspect"]) == w["first"] and int(e["evaluated"]) == g["evaluated"], f"subject {c}"   # (the second one retires when all suspect)
        assert int(e["peak"]) == g["peak"]
    assert sum(1 for e in down.values() if e["all"] != NEVER) == 6 and down[s["live"][2]]["all"] == NEVER


def test_a_crash_inside_an_accusation_closes_it_stopped():
    """From the lossy run: a subject with an ACCUSED episode open over the sample of some tick T (nobody named it beforehand).
    The same run with a crash of it injected at T: the episode closes STOPPED and a DOWN episode opens in the same sample."""
    _, _, _, log, _ = oracle_run("lossy")
    acc = [e for e in log if e["kind"] == _ffi.DETECT_ACCUSED and e["flags"] == 0 and int(e["closed"]) - int(e["opened"]) >= 4]
    assert acc, "no accusation of a bystander that lasts four samples"
    e = acc[0]
    subject, t = int(e["subject"]), int(e["opened"]) + 1         # open over the sample behind tick t (now = t + 1)
    assert int(e["opened"]) < t + 1 < int(e["closed"])
    o2, m2, hdr2, log2, open2 = oracle_run("lossy", extra=((t, _ffi.OP_CRASH, subject),))
    mine = [x for x in log2 if x["subject"] == subject]
    stopped = [x for x in mine if x["outcome"] == _ffi.DETECT_STOPPED]
    assert len(stopped) == 1 and int(hdr2["closed"][-1][_ffi.DETECT_STOPPED - 1]) == 1
    x = stopped[0]
    assert (int(x["kind"]), int(x["opened"]), int(x["closed"]), int(x["evaluated"])) == (_ffi.DETECT_ACCUSED, int(e["opened"]), t + 1, t - int(e["opened"]) + 1)
    downs = [y for y in list(log2) + list(open2) if y["subject"] == subject and y["kind"] == _ffi.DETECT_DOWN]
    assert len(downs) == 1 and int(downs[0]["opened"]) == t + 1 and int(downs[0]["slot"]) == int(x["slot"]) and int(downs[0]["flags"]) == 0
    assert int(downs[0]["first_suspect"]) == t + 1                # it was suspected already
    i = t                                                         # the sample with tick word t + 1
    assert int(hdr2["tick"][i]) == t + 1 and int(hdr2["closed_now"][i]) >= 1
    assert int(hdr2["opened_down"][i]) >= int(hdr2["opened_down"][i - 1]) + 1     # (a scheduled crash may fall on the same tick)
    check_consistent(hdr2, log2, open2)
