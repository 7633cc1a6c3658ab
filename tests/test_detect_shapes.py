"""The detection log (include/serf_sim_detect.h) where its one kernel can be wrong by one without faulting: the part that needs no
GPU.  detect_kernel is the only observer kernel whose output depends on an ORDER computed across lanes, waves and chunks: a
record's place in the log is the log's length before the sample, plus the closes of the chunks before (`base`), of the waves
before (`wcnt[]`) and of the lanes before (two ballots, ">= 1" and "== 2").  This file owns the scenarios that reach that
arithmetic and the conditions that make them non-trivial, and runs them on the CPU oracle with tests/detect_model.py;
tests/test_detect_shapes_gpu.py drives the HIP library through the same scripts and compares word for word.  Which size and
which scenario is there for which guard of the kernel: profiles/detect_shapes.md.

All handles are dense (view_slots = 0): slot == node id and the range of the walk is N.

  ragged(n)     tests/test_observer_shapes.ragged_script at 1 .. 1025 slots: partial waves, a chunk of one lane, `a < p.range`
  double        14 victims crash, are revived (and stay accused: they never hear of their death) and crash again: each closes
                STOPPED and DETECTED in ONE sample — r2, the second ballot — in all four waves of a chunk and in three chunks
  straddle      the same at 300 nodes with a log of 15 records: a pair across the end of the log (`pos + 1 < logcap`); of 14: the
                end falls between two slots (the control); of 16: the pair is the last that fits
  nobody_runs   every node crashes: R == 0, the `if (R)` guard — without it `gone == R` holds with 0 == 0
  resumed       a log, a spread map and a traffic meter STARTED on a handle that sim_restore rebuilt (tests/test_observer_resume.py
                has this for the four older observers), against the models started at tick T on an oracle that never restored
  seven         series, census, roll, ledger, detection log, spread map and traffic meter with two trackers on one handle

Everything compared is an exact integer.  The figures below were measured on this tree's oracle."""
import functools

import numpy as np
import pytest

from serf_amd import _ffi
from tests import test_ledger as tl
from tests import test_observer_resume as rs
from tests import test_observer_shapes as sh
from tests import test_track_gpu as tt
from tests._oracle import load_oracle
from tests.census_model import CensusModel
from tests.detect_model import DetectModel
from tests.ledger_model import LedgerModel
from tests.roll_model import RollModel
from tests.series_model import SeriesModel
from tests.spread_model import SpreadModel
from tests.test_detect import check_consistent
from tests.track_model import TrackModel
from tests.traffic_model import TrafficModel

NEVER = _ffi.DETECT_NEVER
DOWN, ACCUSED = _ffi.DETECT_DOWN, _ffi.DETECT_ACCUSED
DETECTED, STOPPED = _ffi.DETECT_DETECTED, _ffi.DETECT_STOPPED
CENSORED = _ffi.DETECT_F_CENSORED
BLOCK = sh.BLOCK                              # detect_kernel's chunk: one workgroup of BLOCK lanes, four waves
LOG_CAPACITY = 1024


def none(spec):
    """The scripts register trackers through add(spec); the log needs none."""
    return None


def make(n, kw):
    return _ffi.Sim(load_oracle(), _ffi.make_config(n, **kw))


def model_of(m):
    return m.read(), m.log(), m.open()


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def model_run(n, kw, script, ticks, log_capacity=LOG_CAPACITY):
    """script(sim, step) on a fresh oracle with the model behind every tick: dict(o, m, want=(headers, log, open episodes))."""
    o = make(n, kw)
    m = DetectModel(o)
    m.start(0, 1, ticks, log_capacity)
    script(o, m.step)
    cs = o.cluster_stats()
    assert o.tick == ticks and cs["overflow"] == 0 and cs["ops_dropped"] == 0      # the run stays inside the model's bounds
    assert m.count() == (ticks, 0)
    return dict(o=o, m=m, want=model_of(m))


# ---- 1. ragged ranges ----
RAGGED_SIZES = (1, 2, 3, 63, 64, 65, 127, 255, 256, 257, 513, 1025)
RAGGED_TICKS = sh.RAGGED_TICKS
# n = 1025, dense, costs about 12 s of Python model: kRandomNodes only.  (The fan-out model decides who talks to whom; the walk
# of the slots does not know it — and every other size runs under both.)
RAGGED_CASES = [(n, fan) for n in RAGGED_SIZES for fan in sorted(sh.FANOUTS) if n != 1025 or fan == "krandomnodes"]
ONE_LANE_CHUNK = (257, 513, 1025)            # the crashed node n - 1 is the only lane of the last chunk
# measured on the oracle, every size >= 3, both fan-out models: the crashed node's episode opens at 5; the leaver's opens and
# closes in the sample with tick word 73 (nobody ever suspected it: first_suspect NEVER, bin 15 of hist_suspect)
RAGGED_CRASH_OPENED, RAGGED_LEAVE_SAMPLE = 5, 73


def ragged_kw(n, fan):
    return dict(sh.ragged_kw(n, fan), view_slots=0)


def ragged_drive(n):
    return lambda sim, step: sh.ragged_script(sim, n, none, step)


@functools.lru_cache(maxsize=None)
def ragged_oracle(n, fan):
    """Once per session; nobody changes what it returns."""
    return model_run(n, ragged_kw(n, fan), ragged_drive(n), RAGGED_TICKS)


def check_ragged(n, run):
    """The scenario closes what it is for: in the LAST lanes of the range."""
    hdr, log, opened = run["want"]
    assert (hdr["subjects"] == n).all() and hdr["tick"].tolist() == list(range(1, RAGGED_TICKS + 1))
    assert hdr["running"][0] == n and hdr["running"][-1] == max(1, n - 2)
    assert len(opened) == 0
    got = sorted((int(e["slot"]), int(e["subject"]), int(e["kind"]), int(e["outcome"]), int(e["opened"])) for e in log)
    if n == 1:
        assert len(log) == 0 and not hdr["opened_down"].any() and not hdr["opened_accused"].any()
        return
    crash = (n - 1, n - 1, DOWN, DETECTED, RAGGED_CRASH_OPENED)
    if n == 2:
        assert got == [crash]
        return
    assert got == [(n - 2, n - 2, DOWN, DETECTED, RAGGED_LEAVE_SAMPLE), crash]
    leave = log[log["slot"] == n - 2][0]
    assert int(leave["closed"]) == RAGGED_LEAVE_SAMPLE and int(leave["first_suspect"]) == NEVER and int(leave["evaluated"]) == 1
    assert int(hdr["hist_suspect"][-1][15]) == 1 and int(hdr["hist_suspect"][-1].sum()) == 2
    assert hdr["closed"][-1].tolist() == [2, 0, 0, 0, 0]
    if n in ONE_LANE_CHUNK:
        assert (n - 1) % BLOCK == 0
    check_consistent(hdr, log, opened)


@pytest.mark.parametrize("n,fan", RAGGED_CASES)
def test_ragged_closes_in_the_last_lanes_on_the_oracle(n, fan):
    check_ragged(n, ragged_oracle(n, fan))


def test_the_ragged_sizes_are_the_issue_s():
    assert [n for n, fan in RAGGED_CASES if fan == "krandomnodes"] == list(RAGGED_SIZES)
    assert [n for n, fan in RAGGED_CASES if fan == "bijection"] == list(RAGGED_SIZES[:-1])
    assert all(ragged_kw(n, fan)["view_slots"] == 0 for n, fan in RAGGED_CASES)


# ---- 2. two closes per slot, in every wave and three chunks ----
DOUBLE_N, DOUBLE_TICKS = 600, 160
DOUBLE_KW = dict(fanout=3, event_ring=64, query_ring=64, probe_interval=2, view_slots=0)
DOUBLE_VICTIMS = (5, 63, 64, 70, 130, 200, 255, 256, 257, 299, 400, 511, 512, 599)
CRASH, REVIVE, AGAIN = 3, 120, 130
# measured on the oracle: every victim is declared by tick 40; revived at 120 it is accused from the sample 121 on; the sample
# with tick word 131 closes 28 episodes; at the end `closed` by outcome is
DOUBLE_DETECTED_BY, DOUBLE_ACCUSED_FROM, DOUBLE_SAMPLE, DOUBLE_CLOSED_NOW = 40, REVIVE + 1, AGAIN + 1, 28
DOUBLE_CLOSED = [28, 0, 0, 14, 0]


def double_drive(victims, ticks, extra=()):
    def run(sim, step):
        for v in victims:
            sim.inject(CRASH, _ffi.OP_CRASH, v)
            sim.inject(REVIVE, _ffi.OP_REVIVE, v)
            sim.inject(AGAIN, _ffi.OP_CRASH, v)
        for t, op, node in extra:
            sim.inject(t, op, node)
        step(ticks)
    return run


@functools.lru_cache(maxsize=None)
def double_oracle():
    return model_run(DOUBLE_N, DOUBLE_KW, double_drive(DOUBLE_VICTIMS, DOUBLE_TICKS), DOUBLE_TICKS)


def check_pairs(log, victims, first):
    """log[first : first + 2 * len(victims)] is, in ascending slot order, each victim's STOPPED then DETECTED of the sample with
    tick word DOUBLE_SAMPLE."""
    pairs = log[first:first + 2 * len(victims)]
    assert pairs["slot"].tolist() == [v for v in victims for _ in (0, 1)] == pairs["subject"].tolist()
    assert pairs["outcome"].tolist() == [STOPPED, DETECTED] * len(victims)
    assert pairs["kind"].tolist() == [ACCUSED, DOWN] * len(victims)
    assert (pairs["closed"] == DOUBLE_SAMPLE).all()
    assert pairs["opened"].tolist() == [DOUBLE_ACCUSED_FROM, DOUBLE_SAMPLE] * len(victims)


def check_double(run):
    hdr, log, opened = run["want"]
    v = list(DOUBLE_VICTIMS)
    assert v == sorted(v) and len(v) == 14
    assert {x // 64 % 4 for x in v if x < BLOCK} == {0, 1, 2, 3}, "a victim in every wave of the first chunk"
    assert {x // BLOCK for x in v} == {0, 1, 2}, "victims in three chunks"
    assert {63, 64, 255, 256, 511, 512, DOUBLE_N - 1} <= set(v), "both sides of the wave and chunk boundaries, and the last lane"
    early = log[log["closed"] <= DOUBLE_DETECTED_BY]
    assert sorted(early["subject"].tolist()) == v and (early["outcome"] == DETECTED).all() and len(log) == 14 + 28
    assert int(hdr["tick"][DOUBLE_SAMPLE - 1]) == DOUBLE_SAMPLE and int(hdr["closed_now"][DOUBLE_SAMPLE - 1]) == DOUBLE_CLOSED_NOW
    assert int(hdr["closed_now"].sum()) == 14 + 28 and int(hdr["closed_now"].max()) == 28
    at = np.nonzero(log["closed"] == DOUBLE_SAMPLE)[0]
    assert at.tolist() == list(range(14, 14 + 28)), "the 28 records are consecutive in the log"
    check_pairs(log, v, 14)
    for x in v:                                          # two records with the same (slot, closed)
        mine = log[(log["slot"] == x) & (log["closed"] == DOUBLE_SAMPLE)]
        assert len(mine) == 2
    assert hdr["closed"][-1].tolist() == DOUBLE_CLOSED and len(opened) == 0
    assert (hdr["open_accused"][DOUBLE_ACCUSED_FROM - 1:DOUBLE_SAMPLE - 1] == 14).all()
    check_consistent(hdr, log, opened)


def test_two_closes_per_slot_in_every_wave_and_three_chunks_on_the_oracle():
    check_double(double_oracle())


# ---- 3. a pair across the end of the log ----
STRADDLE_N, STRADDLE_TICKS = 300, 200
STRADDLE_VICTIMS = tuple(v for v in DOUBLE_VICTIMS if v < STRADDLE_N)
STRADDLE_LATE = (140, _ffi.OP_CRASH, 7)      # one more crash: its DETECTED closes after the log is full
STRADDLE_ODD, STRADDLE_EVEN, STRADDLE_FITS = 15, 14, 16
# capacity -> ((slot, outcome) of the last record written, of the first one lost): the end of the log inside slot 64's pair; between
# slots 63 and 64 (the control); right behind slot 64's pair.  14 and 16 are the capacities at which the SECOND record of a pair
# is the log's last: there `pos + 1 < logcap` holds by one.  The order is the order the GPU tests run in, 15 last: the library
# does not clear a new log, and a test of a record that a wrong bound leaves unwritten must not find, in memory that an
# earlier handle gave back, the very record of the same run with another capacity.
STRADDLE_ENDS = {STRADDLE_EVEN: ((63, DETECTED), (64, STOPPED)), STRADDLE_FITS: ((64, DETECTED), (70, STOPPED)),
                 STRADDLE_ODD: ((64, STOPPED), (64, DETECTED))}
STRADDLE_CAPS = tuple(STRADDLE_ENDS)
# measured on the oracle with capacity 1024: 31 records — 10 before the sample with tick word 131, 20 in it, 1 after
STRADDLE_RECORDS, STRADDLE_BEFORE, STRADDLE_IN = 31, 10, 20


@functools.lru_cache(maxsize=None)
def straddle_oracle(log_capacity):
    return model_run(STRADDLE_N, DOUBLE_KW, double_drive(STRADDLE_VICTIMS, STRADDLE_TICKS, (STRADDLE_LATE,)), STRADDLE_TICKS, log_capacity)


def check_straddle(cap, run, full):
    (hdr, log, opened), (fh, fl, fo) = run["want"], full["want"]
    v = list(STRADDLE_VICTIMS)
    assert len(v) == 10 and len(fl) == STRADDLE_RECORDS
    assert int((fl["closed"] < DOUBLE_SAMPLE).sum()) == STRADDLE_BEFORE and int((fl["closed"] == DOUBLE_SAMPLE).sum()) == STRADDLE_IN
    check_pairs(fl, v, STRADDLE_BEFORE)
    late = fl[-1]
    assert (int(late["subject"]), int(late["outcome"]), int(late["opened"])) == (7, DETECTED, STRADDLE_LATE[0] + 1) and int(late["closed"]) > DOUBLE_SAMPLE
    check_consistent(fh, fl, fo)
    # the short log: the prefix of the full one; the counters and histograms go on
    assert run["m"].log_count() == (cap, STRADDLE_RECORDS - cap) and same(log, fl[:cap])
    last, lost = log[-1], fl[cap]            # (capacity 15: record 14 is slot 64's STOPPED; its DETECTED is lost)
    assert ((int(last["slot"]), int(last["outcome"])), (int(lost["slot"]), int(lost["outcome"]))) == STRADDLE_ENDS[cap]
    assert int(last["closed"]) == int(lost["closed"]) == DOUBLE_SAMPLE
    i = DOUBLE_SAMPLE - 1                     # the samples with tick words 130, 131, 132
    assert hdr["tick"][i - 1:i + 2].tolist() == [130, 131, 132]
    assert hdr["log_written"][i - 1:i + 2].tolist() == [STRADDLE_BEFORE, cap, cap]
    assert hdr["log_lost"][i - 1:i + 2].tolist() == [0, STRADDLE_BEFORE + STRADDLE_IN - cap, STRADDLE_BEFORE + STRADDLE_IN - cap]
    j = int(late["closed"]) - 1               # the late DETECTED of node 7 is lost as well
    assert hdr["log_lost"][j - 1:j + 1].tolist() == [STRADDLE_RECORDS - 1 - cap, STRADDLE_RECORDS - cap]
    assert (hdr["log_written"] == np.minimum(fh["log_written"], cap)).all() and (hdr["log_lost"] == fh["log_written"] - hdr["log_written"]).all()
    for f in ("closed", "false_declared", "opened_down", "opened_accused", "hist_suspect", "hist_all", "hist_cleared", "closed_now",
              "open_down", "open_accused", "running", "subjects", "tick"):
        assert same(hdr[f], fh[f]), f
    assert same(opened, fo)
    check_consistent(hdr, log, opened, lost=STRADDLE_RECORDS - cap)


@pytest.mark.parametrize("cap", STRADDLE_CAPS)
def test_a_pair_across_the_end_of_the_log_on_the_oracle(cap):
    check_straddle(cap, straddle_oracle(cap), straddle_oracle(LOG_CAPACITY))
    if cap == STRADDLE_ODD:
        assert straddle_oracle(cap)["m"].log_count() == (15, 16)


# ---- 4. nobody runs ----
IDLE_CASES = [(n, fan) for n in sh.IDLE_SIZES for fan in sorted(sh.FANOUTS)]


def idle_kw(fan):
    return dict(sh.KW, view_slots=0, flags=sh.FANOUTS[fan])


def idle_drive(n):
    return lambda sim, step: sh.idle_script(sim, n, none, step)


@functools.lru_cache(maxsize=None)
def idle_oracle(n, fan):
    return model_run(n, idle_kw(fan), idle_drive(n), sh.IDLE_TICKS)


def check_idle(n, run):
    hdr, log, opened = run["want"]
    late = sh.IDLE_TICKS - sh.IDLE_CRASH
    assert hdr["running"].tolist() == [n] * sh.IDLE_CRASH + [0] * late
    assert int((hdr["running"] == 0).sum()) >= 6, "R == 0 in at least six samples"
    assert hdr["open_down"].tolist() == [0] * sh.IDLE_CRASH + [n] * late
    assert int(hdr["closed"].sum()) == 0 and not hdr["closed_now"].any() and len(log) == 0, "nothing ever closes"
    assert len(opened) == n and opened["slot"].tolist() == list(range(n)) and (opened["kind"] == DOWN).all()
    assert (opened["opened"] == sh.IDLE_CRASH + 1).all() and (opened["evaluated"] == late).all()
    for f in ("half", "p99", "all"):
        assert (opened[f] == NEVER).all(), f
    check_consistent(hdr, log, opened)


@pytest.mark.parametrize("n,fan", IDLE_CASES)
def test_nobody_runs_on_the_oracle(n, fan):
    check_idle(n, idle_oracle(n, fan))


# ---- 5. observers started on a restored handle ----
RESUMED_N = 65                              # rs.ragged_run(65, fan): node 64, the one lane of the second wave, is down in the image


def never_restored(case, setup, model, start):
    """The reference: model(o) on an oracle that runs the case from tick 0 and never restores; the observer starts at tick T."""
    o = case.make()
    case.before(o)
    m = model(o)
    m.step(case.T)                          # (not started yet: the model only follows the run)
    assert o.tick == case.T
    start(m)
    case.after(o, m.step, setup)
    assert o.tick == case.ticks
    tl.inside_bounds(o)
    return o, m


@functools.lru_cache(maxsize=None)
def resumed_detect_oracle(fan):
    case, img, cond, ref = rs.ragged_run(RESUMED_N, fan)
    o, m = never_restored(case, ref["setup"], DetectModel, lambda m: m.start(0, 1, case.ticks, LOG_CAPACITY))
    return dict(o=o, m=m, want=model_of(m))


def check_resumed_detect(fan, run):
    case, img, cond, ref = rs.ragged_run(RESUMED_N, fan)
    hdr, log, opened = run["want"]
    T, n = case.T, case.n
    assert run["m"].count() == (case.ticks - T, 0) and hdr["tick"].tolist() == list(range(T + 1, case.ticks + 1))
    assert int(hdr["open_down"][0]) >= 1 and int(hdr["opened_down"][0]) >= 1, "a subject is down in the image"
    cens = log[(log["flags"] & CENSORED) != 0]
    assert cens["subject"].tolist() == [n - 1] and cens["opened"].tolist() == [T + 1] and cens["outcome"].tolist() == [DETECTED]
    assert [int(e["subject"]) for e in log if not e["flags"] & CENSORED] == [n - 2], "the leaver's episode opens later: not censored"
    assert int(hdr["hist_all"][-1].sum()) == 1                  # the censored one stays out of the histograms
    assert run["o"].digest() == ref["end"]["digest"]
    check_consistent(hdr, log, opened)


@pytest.mark.parametrize("fan", sorted(sh.FANOUTS))
def test_a_log_started_at_the_image_s_tick_opens_censored_on_the_oracle(fan):
    check_resumed_detect(fan, resumed_detect_oracle(fan))


def resumed_entries(setup, n):
    return list(dict.fromkeys(sh.five_rumours(setup["ru"], n)))


@functools.lru_cache(maxsize=None)
def resumed_spread_oracle(fan="krandomnodes"):
    case, img, cond, ref = rs.ragged_run(RESUMED_N, fan)
    entries = resumed_entries(ref["setup"], case.n)
    o, m = never_restored(case, ref["setup"], SpreadModel, lambda m: m.start(entries, 0, 1, case.ticks))
    return dict(o=o, m=m, entries=entries, samples=m.read())


def check_resumed_spread(run, fan="krandomnodes"):
    case, img, cond, ref = rs.ragged_run(RESUMED_N, fan)
    hdr, rec = run["samples"]
    assert hdr["tick"].tolist() == list(range(case.T + 1, case.ticks + 1))
    kinds = [e[0] for e in run["entries"]]
    assert set(kinds) == {_ffi.K_JOIN, _ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY}
    ev = kinds.index(_ffi.K_EVENT)
    assert rec["new"][0, ev] > 1, "nodes that held the event in the image are latched at the first sample"
    assert rec["first"][-1, ev] == case.T + 1
    assert rec["reached"][-1].max() == case.n - 1, "the node that is down in the image never has an arrival"
    assert run["o"].digest() == ref["end"]["digest"]


def test_a_spread_map_started_at_the_image_s_tick_on_the_oracle():
    check_resumed_spread(resumed_spread_oracle())


@functools.lru_cache(maxsize=None)
def resumed_traffic_oracle(fan="bijection"):
    case, img, cond, ref = rs.ragged_run(RESUMED_N, fan)
    o, m = never_restored(case, ref["setup"], TrafficModel, lambda m: m.start(0, 1, case.ticks))
    return dict(o=o, m=m)


def check_resumed_traffic(run, fan="bijection"):
    case, img, cond, ref = rs.ragged_run(RESUMED_N, fan)
    s = run["m"].read()
    assert s["tick"].tolist() == list(range(case.T + 1, case.ticks + 1))
    assert s["packets"][0] > 0, "the first sample counts the packets in flight of the image"
    assert cond["in_flight"] > 0 and s["running"][0] == case.n - 1
    assert run["o"].digest() == ref["end"]["digest"]


def test_a_traffic_meter_started_at_the_image_s_tick_on_the_oracle():
    check_resumed_traffic(resumed_traffic_oracle())


# ---- 6. all seven observers and two trackers on one handle ----
SEVEN_N, SEVEN_TICKS, SEVEN_TOP_K = 4096, 160, 8
SEVEN_KW = dict(tt.KW, flags=tt.KRANDOM)     # the cluster and the script of test_ledger_gpu.test_all_five_observers_on_one_handle
SEVEN_PERIODS = dict(series=1, census=2, roll=3, ledger=1, detect=1, spread=2, traffic=3)


def seven_script(sim, add, step, ticks=SEVEN_TICKS):
    """tt.drive's script — six crashes, forty user events, one step(k) per stretch between two injections — with two trackers:
    "the first crash is suspected or worse" and the first event.  Returns ([tracker handles], the events as (kind, key, ltime))."""
    s = tt.script(SEVEN_N)
    for t, c in zip(s["crash_at"], s["crashed"]):
        sim.inject(t, _ffi.OP_CRASH, c)
    handles = [add(_ffi.member_tracker(s["crashed"][0], tt.FAILED, tt.SUSPECT_OR_DEAD, start=s["crash_at"][0]))]
    events = []
    for te, node, key in s["events"]:
        if te >= ticks:
            break
        step(te - sim.tick)
        events.append((_ffi.K_EVENT, key, int(sim.stats(node).event_time)))
        if len(events) == 1:
            handles.append(add(_ffi.rumour_tracker(*events[0])))
        sim.user_event(node, key, 64)
    step(ticks - sim.tick)
    return handles, events


@functools.lru_cache(maxsize=None)
def seven_entries():
    """(the ledger's entries, the spread map's) — the events' Lamport times from a dry run."""
    dry = make(SEVEN_N, SEVEN_KW)
    _, events = seven_script(dry, none, dry.step)
    dry.close()
    s = tt.script(SEVEN_N)
    ledger = events + [(_ffi.K_SUSPECT, c, 0) for c in s["crashed"]] + [(_ffi.K_DEAD, c, 0) for c in s["crashed"]]
    spread = events[:6] + [(_ffi.K_JOIN, s["crashed"][0], 1), (_ffi.K_JOIN, s["live"][0], 1)]
    assert len(ledger) <= _ffi.LEDGER_MAX
    return ledger, spread


def seven_start(starts, capacity=SEVEN_TICKS):
    """starts: {name: start function of a model or of the handle}; the same arguments for both sides."""
    ledger, spread = seven_entries()
    p = SEVEN_PERIODS
    starts["series"](0, p["series"], capacity)
    starts["census"](0, p["census"], capacity, 64)
    starts["roll"](0, p["roll"], capacity, SEVEN_TOP_K, _ffi.ROLL_BY_ACCUSED)
    starts["ledger"](ledger, 0, p["ledger"], capacity)
    starts["detect"](0, p["detect"], capacity, LOG_CAPACITY)
    starts["spread"](spread, 0, p["spread"], capacity)
    starts["traffic"](0, p["traffic"], capacity)


@functools.lru_cache(maxsize=None)
def seven_oracle():
    o = make(SEVEN_N, SEVEN_KW)
    tm = TrackModel(o)
    ms = dict(census=CensusModel(o), roll=RollModel(o), ledger=LedgerModel(o), detect=DetectModel(o), spread=SpreadModel(o), traffic=TrafficModel(o))

    followers = list(ms.values())

    def behind():
        tm.evaluate()
        for m in followers:
            m.after_tick(o.tick - 1)
    ms["series"] = SeriesModel(o, behind)
    seven_start({k: m.start for k, m in ms.items()})
    handles, events = seven_script(o, tm.add, ms["series"].step)
    tl.inside_bounds(o)
    return dict(o=o, models=ms, trackers=[tm.result(h) for h in handles], events=events)


def check_seven(run):
    ms, t = run["models"], SEVEN_TICKS
    assert run["events"] == seven_entries()[0][:len(run["events"])]
    for name, period in SEVEN_PERIODS.items():
        assert ms[name].count() == (len(range(0, t, period)), 0), name
    hdr, log, opened = model_of(ms["detect"])
    assert int(hdr["closed"][-1][DETECTED - 1]) == 6 and len(log) >= 6, "every crash is detected inside the run"
    assert ms["spread"].read()[1]["reached"][-1].min() > SEVEN_N // 2 and ms["traffic"].read()["packets"].sum() > 0
    member, event = run["trackers"]
    assert member["all"] != _ffi.TRACK_NEVER and event["all"] != _ffi.TRACK_NEVER
    check_consistent(hdr, log, opened)


def test_all_seven_observers_on_the_oracle():
    check_seven(seven_oracle())
