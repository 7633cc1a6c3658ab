"""Query board (include/serf_sim_qboard.h), the part that needs no GPU: the extension's interface next to the ABI and the nine
extensions it must not disturb, the reference model (tests/qboard_model.py) against independent routes on the oracle —
sim_query_status at every tick, the spread model's arrivals of the same query, the running-query section of the checkpoint image —
the invariants of the samples, the latch, displacement and restart rules, and qboard_summary on a hand-made array.

This file owns the scenarios that tests/test_qboard_gpu.py runs on the GPU as well.  A scenario is a function of a Script
(tests/qboard_model.py): it schedules every operation up front.  Everything compared is an exact integer."""
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
from tests import test_snapshot as tsn
from tests import test_tree as tt
from tests._oracle import load_oracle
from tests.qboard_model import CLOSED, DISPLACED, EW, HW, OPEN, WAITING, QBoardModel, Script, q_timeout
from tests.spread_model import SpreadModel
from tests.test_track_gpu import BIJECTION, KRANDOM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QBOARD_HEADER = os.path.join(ROOT, "include", "serf_sim_qboard.h")
QBOARD_INC = os.path.join(ROOT, "serf_amd", "csrc", "serf_sim_qboard.inc")
ACK, RESP = _ffi.F_ACK, _ffi.F_RESPOND
KW = dict(fanout=3, view_slots=16, event_ring=64, query_ring=64, flags=KRANDOM)
QBOARD_GRID, BLOCK = 1024, 256                  # serf_sim_qboard.inc: #define QBOARD_GRID 1024u; serf_sim.hip: #define BLOCK 256


def relay(k):
    return k << 8                               # QueryMessage.relay_factor in the flags (include/serf_sim.h)


def make(n, kw):
    return _ffi.Sim(load_oracle(), _ffi.make_config(n, **kw))


def model_run(n, kw, scenario, ids, ticks, first=0, period=1, capacity=1 << 12, before=0, on_tick=None):
    """The scenario on a fresh oracle, `before` ticks without a board, then the model's board behind `ticks` more.  Returns
    dict(o, m, script, ids, samples)."""
    o = make(n, kw)
    sc = Script(o)
    scenario(sc)
    m = QBoardModel(o, sc, on_tick)
    m.step(before)
    m.start(ids, first, period, capacity)
    m.step(ticks)
    return dict(o=o, m=m, script=sc, ids=list(ids), samples=m.read())


# ---- 1. the full scenario: table edges, filters, tags, crashes, a displacement, a restart ----
FULL_IDS = [256, 255, 5, 261, 999]              # residues 0, 255, 5, 5 again; 999 is never scheduled
FULL_SIZES = (33, 64, 65, 96, 97, 257)
FILTER_12 = lambda n: sorted({0, n - 1, n // 2, *range(3, 3 + 12)} & set(range(n)))[:12]


def full_ticks(n):
    return 2 * q_timeout(n) + 8


def full_kw(n, fan=KRANDOM):
    return dict(KW, flags=fan, loss=0.1)


def full(sc, n):
    """Query 256 (residue 0) asks everybody for an ack and a response; 255 (residue 255) asks tag classes 1 and 2 for an ack and
    loses its origin; 5 asks twelve nodes by id with relay_factor 3, loses its filter record to 261 at tick 10 and its table entry
    at tick 14; 256 is issued again behind its deadline.  Node 4 changes its class while 255 is open; nodes 3 and n - 1 crash
    with their answers in."""
    t = q_timeout(n)
    sc.init_tags([1 + x % 3 if x % 2 == 0 else 0 for x in range(n)])
    sc.query(1, n // 2, 256, ACK | RESP)
    sc.query(2, 1, 255, ACK, mask=0b0110)
    sc.query(3, 2, 5, ACK | RESP | relay(3), ids=FILTER_12(n))
    sc.inject(4, _ffi.OP_SET_TAGS, 4, 3)        # class 2 -> 3: no longer admitted by 255
    sc.inject(4, _ffi.OP_SET_TAGS, 1, 1)        # class 0 -> 1: admitted from now on
    sc.inject(6, _ffi.OP_CRASH, 3)
    sc.inject(6, _ffi.OP_CRASH, n - 1)
    sc.inject(7, _ffi.OP_SET_TAGS, 3, 1)        # a node that does not run: the class is stored all the same
    sc.inject(5, _ffi.OP_CRASH, 1)              # the origin of 255, before its deadline
    for x in (10, n // 3, n - 2):
        sc.inject(12, _ffi.OP_CRASH, x)         # ... and three more once the answers are in
    sc.inject(10, _ffi.OP_QUERY_FILTER_ID, 0, 261, 7)
    sc.inject(14, _ffi.OP_QUERY, 0, 261, ACK)
    sc.inject(t + 5, _ffi.OP_QUERY, 0, 256, ACK)


@functools.lru_cache(maxsize=None)
def full_run(n, fan=KRANDOM, **start):
    return model_run(n, full_kw(n, fan), lambda sc: full(sc, n), FULL_IDS, full_ticks(n) - start.get("before", 0), **start)


def check_full(n, run):
    """The scenario shows what it is for."""
    hdr, rec = run["samples"]
    t = q_timeout(n)
    by = {qid: rec[:, i] for i, qid in enumerate(FULL_IDS)}
    assert (by[999]["state"] == WAITING).all() and not np.ascontiguousarray(by[999]).view(np.uint64).reshape(-1, EW)[:, 1:].any()
    assert by[256]["state"].tolist()[:t + 6] == [WAITING] + [OPEN] * t + [CLOSED] * 4 + [OPEN]
    assert by[256]["origin"][1] == n // 2 and by[256]["origin"][-1] == 0 and by[256]["deadline"][-1] == 2 * t + 5
    assert 0 < by[256]["t_first"][t + 4] <= 4 and by[256]["t_first"][t + 5] in (0, t + 6) and by[256]["t_first"][-1] > t + 5
    assert (by[256]["acks"] > by[256]["answered"]).any(), "no answered node crashed"
    assert by[255]["eligible"].max() < n and by[255]["acks"][-1] < by[255]["eligible"].max(), "255's origin crashed early"
    assert by[5]["state"].tolist()[:14] == [WAITING] * 3 + [OPEN] * 11 and (by[5]["state"][14:] == DISPLACED).all()
    assert by[5]["eligible"][8] <= 12 and by[5]["eligible"][10] == hdr["running"][10], "behind tick 10 the filter record is 261's"
    assert by[5]["deadline"][-1] == 3 + t and not by[5]["acks"][14:].any()
    assert by[261]["state"].tolist()[:15] == [WAITING] * 14 + [OPEN] and by[261]["eligible"].max() == 1, "261 asks node 7 alone"
    assert hdr["displaced"][-1] == 1 and hdr["waiting"][-1] == 1 and hdr["closed"][-1] == 3 and hdr["open"][-1] == 0


@pytest.mark.parametrize("n", FULL_SIZES)
def test_the_full_scenario_is_nontrivial_on_the_oracle(n):
    check_full(n, full_run(n))


# ---- 2. further scenarios ----
def tiny(sc):
    """Three nodes, relay_factor 7: N < relay + 1, no relays."""
    sc.query(1, 1, 9, ACK | RESP | relay(7))


TINY = (3, dict(KW, view_slots=3, fanout=2, loss=0.3), tiny, [9, 265], 24)

CROWD_N, CROWD_TICKS = 97, 50
CROWD_IDS = [7 * i + 1 for i in range(48)] + [256 + 7 * i + 1 for i in range(16)]    # 64 entries; the last 16 share the first 16's residues


def crowd(sc):
    """64 entries, every third never scheduled; the others one every tick from varying origins with varying flags."""
    for i, qid in enumerate(CROWD_IDS):
        if i % 3 != 2:
            sc.query(1 + i // 2, (5 * i) % CROWD_N, qid, (ACK, ACK | RESP, RESP)[i % 3 if i % 3 < 2 else 0] | relay(i % 4),
                     ids=[(11 * i + k) % CROWD_N for k in range(i % 5)] or None)


CROWD = (CROWD_N, dict(KW, loss=0.05), crowd, CROWD_IDS, CROWD_TICKS)

IDLE_N, IDLE_TICKS = 64, 10


def idle(sc):
    """Everybody crashes behind tick 3: nobody is eligible, the bits stay."""
    sc.query(1, 5, 300, ACK | RESP)
    for x in range(IDLE_N):
        sc.inject(4, _ffi.OP_CRASH, x)


IDLE = (IDLE_N, dict(KW), idle, [300, 44], IDLE_TICKS)

LATE_N = 64


def late(sc):
    """Query 77 asks tag class 1 — nodes 10 and 11 — for an ack.  Node 11 is down while the query travels and comes back when nobody
    sends it any more: it runs, is admitted and stays silent.  Behind the deadline it changes its class: answered == eligible is
    first met in a CLOSED sample, and no latch may move."""
    sc.init_tags([1 if x in (10, 11) else 0 for x in range(LATE_N)])
    sc.inject(0, _ffi.OP_CRASH, 11)
    sc.query(1, 3, 77, ACK, mask=0b10)
    sc.inject(24, _ffi.OP_REVIVE, 11)
    sc.inject(q_timeout(LATE_N) + 4, _ffi.OP_SET_TAGS, 11, 2)


LATE = (LATE_N, dict(KW), late, [77], q_timeout(LATE_N) + 8)

LOSS_N = 4096
LOSS_VARIANTS = [(r, fan) for r in (0, 3) for fan in ("krandomnodes", "bijection")]


def lossy(sc, relay_factor):
    sc.query(1, 17, 700, ACK | RESP | relay(relay_factor))
    sc.query(3, 4000, 701, ACK | relay(relay_factor), mask=0b10)


def loss_kw(fan):
    return dict(KW, view_slots=32, loss=0.3, flags=KRANDOM if fan == "krandomnodes" else BIJECTION)


@functools.lru_cache(maxsize=None)
def loss_run(relay_factor, fan):
    def scenario(sc):
        sc.init_tags([x % 2 for x in range(LOSS_N)])
        lossy(sc, relay_factor)
    return model_run(LOSS_N, loss_kw(fan), scenario, [700, 701], q_timeout(LOSS_N) + 6)


SECOND_N = QBOARD_GRID * BLOCK + 65             # the size tests/test_spread_gpu.py::test_second_pass uses
SECOND_TICKS, SECOND_PERIOD = 9, 4
SECOND_KW = dict(fanout=4, event_ring=64, query_ring=64, probe_interval=5, loss=0.01, ring_overflow=4, join_sync=True, view_slots=16, flags=KRANDOM)


def second(sc):
    sc.inject(2, _ffi.OP_CRASH, SECOND_N - 1)
    sc.query(1, SECOND_N - 3, 77, ACK | RESP)


@functools.lru_cache(maxsize=None)
def second_pass_run():
    return model_run(SECOND_N, SECOND_KW, second, [77], SECOND_TICKS, period=SECOND_PERIOD, capacity=100)


SMALL = dict(tiny=TINY, crowd=CROWD, idle=IDLE, late=LATE)


@functools.lru_cache(maxsize=None)
def small_run(name):
    n, kw, scenario, ids, ticks = SMALL[name]
    return model_run(n, kw, scenario, ids, ticks)


def test_the_small_scenarios_are_nontrivial_on_the_oracle():
    hdr, rec = small_run("tiny")["samples"]
    assert rec["state"][-1].tolist() == [CLOSED, WAITING] and rec["eligible"].max() == 3 and 0 < rec["acks"][-1, 0] <= 3
    hdr, rec = small_run("crowd")["samples"]
    assert hdr["waiting"][-1] >= 21 and hdr["open"].max() >= 20 and hdr["closed"][-1] >= 10 and hdr["n"][0] == 64
    residues = [q % 256 for q in CROWD_IDS]
    assert len(set(residues)) < 64 and hdr["displaced"][-1] >= 1, "no two scheduled entries share a residue"
    assert (rec["eligible"][-1] > 0).sum() >= 30 and (rec["silent"] > 0).any() and (rec["t_all"][-1] > 0).any()
    hdr, rec = small_run("late")["samples"]
    t = q_timeout(LATE_N)
    col = rec[:, 0]
    assert col["state"].tolist() == [WAITING] + [OPEN] * t + [CLOSED] * 7
    assert col["eligible"].tolist()[20:] == [1] * 4 + [2] * (t - 20) + [1] * 4 and col["answered"].tolist()[20:] == [1] * (t + 8 - 20)
    assert col["t_all"][23] > 0 and col["t_all"][24] == col["t_all"][23], "all of ONE eligible node answered before node 11 came back"
    late_run = model_run(LATE_N, dict(KW), late, [77], t + 8 - 24, before=24)      # a board started behind the revive: nothing latched early
    col = late_run["samples"][1][:, 0]
    assert col["t_half"][0] == 25 and not col["t_all"].any() and not col["t_90"].any(), "a == e is first met behind the deadline: no latch"
    assert (col["answered"][-4:] == col["eligible"][-4:]).all() and (col["state"][-4:] == CLOSED).all()
    hdr, rec = small_run("idle")["samples"]
    assert hdr["running"].tolist() == [IDLE_N] * 4 + [0] * (IDLE_TICKS - 4)
    assert not rec["eligible"][4:].any() and rec["acks"][-1, 0] > 0 and rec["t_all"][-1, 0] == 0 and rec["state"][-1].tolist() == [OPEN, WAITING]


# ---- 3. the model against the library's own figures ----
@pytest.mark.parametrize("n", (65, 257))
def test_words_3_and_4_are_query_status_at_every_tick(n):
    """state_of asserts it inside the model; here the route is walked once more from outside, on a run of its own."""
    seen = []
    ids = FULL_IDS
    o = make(n, full_kw(n))

    def on_tick():
        row = []
        for qid in ids:
            try:
                row.append(o.query_status(qid))
            except _ffi.SimError:
                row.append(None)
        seen.append(row)
    sc = Script(o)
    full(sc, n)
    m = QBoardModel(o, sc, on_tick)
    m.start(ids)
    m.step(full_ticks(n))
    hdr, rec = m.read()
    assert words_of(m.read()) == words_of(full_run(n)["samples"])
    for k, row in enumerate(seen):
        for i, st in enumerate(row):
            if st is None:
                assert rec["state"][k, i] in (WAITING, DISPLACED) and rec["acks"][k, i] == rec["responses"][k, i] == 0
            else:
                assert (rec["acks"][k, i], rec["responses"][k, i], rec["state"][k, i] == OPEN) == st
    o.close()


def words_of(samples):
    return [np.ascontiguousarray(a).view(np.uint64).reshape(-1).tolist() for a in samples]


def all_runs():
    return [full_run(n) for n in FULL_SIZES] + [small_run(x) for x in ("tiny", "crowd", "idle", "late")]


def test_sample_invariants():
    for run in all_runs():
        hdr, rec = run["samples"]
        assert (rec["answered"] + rec["silent"] == rec["eligible"]).all()
        assert (rec["answered"] <= rec["acks"]).all() and (rec["responded"] <= rec["responses"]).all()
        assert (rec["eligible"] <= hdr["running"][:, None]).all()
        assert (hdr["open"] + hdr["closed"] + hdr["waiting"] + hdr["displaced"] == hdr["n"]).all()
        assert hdr["new"].tolist() == (rec["new_acks"] + rec["new_responses"]).sum(axis=1).tolist()
        assert hdr["tick"].tolist() == list(range(1, len(hdr) + 1))
        now = np.broadcast_to(hdr["tick"][:, None], rec.shape)
        assert (now[rec["state"] == OPEN] <= rec["deadline"][rec["state"] == OPEN]).all()
        assert (now[rec["state"] == CLOSED] > rec["deadline"][rec["state"] == CLOSED]).all()


def test_latches_are_set_once_in_order_and_only_while_open():
    for run in all_runs():
        hdr, rec = run["samples"]
        for i in range(rec.shape[1]):
            col = rec[:, i]
            for k in range(1, len(col)):
                same = col["state"][k - 1] in (OPEN, CLOSED, DISPLACED) and col["deadline"][k] == col["deadline"][k - 1] and col["origin"][k] == col["origin"][k - 1]
                for name in ("t_first", "t_half", "t_90", "t_99", "t_all"):
                    if same and col[name][k - 1]:
                        assert col[name][k] == col[name][k - 1], "a latch moved"
                    if col[name][k] and not (same and col[name][k - 1]):
                        assert col[name][k] == hdr["tick"][k] and col["state"][k] == OPEN and col["eligible"][k] > 0
            on = [col[name].astype(np.int64) for name in ("t_first", "t_half", "t_90", "t_99", "t_all")]
            for a, b in zip(on, on[1:]):
                assert ((b == 0) | ((a != 0) & (a <= b))).all(), "a later latch before an earlier one"


def test_displacement_and_restart_rules():
    n = 65
    hdr, rec = full_run(n)["samples"]
    t = q_timeout(n)
    five = rec[:, FULL_IDS.index(5)]
    last_open = five[13]
    for k in range(14, len(five)):
        assert five["state"][k] == DISPLACED and five["origin"][k] == last_open["origin"] and five["deadline"][k] == last_open["deadline"]
        assert [five[x][k] for x in ("t_first", "t_half", "t_90", "t_99", "t_all")] == [last_open[x] for x in ("t_first", "t_half", "t_90", "t_99", "t_all")]
        assert not any(five[x][k] for x in ("acks", "responses", "eligible", "answered", "responded", "silent", "new_acks", "new_responses"))
    again = rec[:, FULL_IDS.index(256)]
    assert 0 < again["t_first"][t + 4] <= 4 and again["acks"][t + 4] > 0
    assert again["acks"][t + 5] == again["new_acks"][t + 5] and again["responses"][t + 5] == 0, "the second query starts from no bits"
    assert again["t_first"][t + 5] in (0, t + 6) and again["t_first"][-1] > t + 5 and again["flags"][-1] == ACK


def test_a_board_started_late_takes_what_is_there_as_new():
    n = 65
    run = full_run(n, before=9)
    hdr, rec = run["samples"]
    ref = full_run(n)["samples"][1]
    assert hdr["tick"][0] == 10 and rec["state"][0].tolist() == [OPEN, OPEN, OPEN, WAITING, WAITING]
    assert rec["new_acks"][0].tolist() == rec["acks"][0].tolist() == ref["acks"][9].tolist() and rec["acks"][0, 0] > 0
    for name in ("acks", "responses", "eligible", "answered", "responded", "silent", "state", "deadline"):
        assert rec[name].tolist() == ref[name][9:].tolist(), name
    assert rec["t_first"][0, 0] == 10 and 0 < ref["t_first"][9, 0] <= 4, "a latch is the first SAMPLE that met the condition"


def test_period_first_tick_and_capacity():
    n, first, period = 65, 7, 3
    ticks = full_ticks(n)
    due = len(range(first, ticks, period))
    run = full_run(n, first=first, period=period, capacity=due - 3)
    hdr, rec = run["samples"]
    assert run["m"].count() == (due - 3, 3) and hdr["tick"].tolist() == [first + 1 + period * i for i in range(due - 3)]
    ref = full_run(n)["samples"][1]
    at = hdr["tick"].astype(np.int64) - 1
    for name in ("acks", "responses", "eligible", "answered", "state"):
        assert rec[name].tolist() == ref[name][at].tolist(), name
    assert rec["new_acks"][1:4, 0].tolist() == np.diff(ref["acks"][at, 0].astype(np.int64)).tolist()[:3], "new: since the previous SAMPLE"
    assert rec["t_first"][0, 0] == first + 1 and (rec["t_half"][:, 0][rec["t_half"][:, 0] > 0] % period == (first + 1) % period).all()


# ---- 4. independent routes ----
CONV_N, CONV_TICKS = 257, 40


def test_t_all_is_the_spread_models_last_arrival_and_answered_is_below_holds():
    """Lossless, unfiltered, nobody crashes: a node's ack reaches the origin in the tick the node first sees the query, so
    `answered` never exceeds the number of nodes that hold the query, and t_all is the tick the last node got it — which the
    spread model latches as `last` — as t_first is its `first`."""
    kw = dict(KW)
    o = make(CONV_N, kw)
    sc = Script(o)
    lt = o.stats(9).query_time
    sc.query(1, 9, 4242, ACK)
    qm = QBoardModel(o, sc)
    sm = SpreadModel(o)
    qm.start([4242])
    sm.start([(_ffi.K_QUERY, 4242, lt)], 0, 1, CONV_TICKS)
    for _ in range(CONV_TICKS):
        t = o.tick
        o.step(1)
        sm.after_tick(t)
        qm.after_tick(t)
    hdr, rec = qm.read()
    shdr, srec = sm.read()
    assert q_timeout(CONV_N) > CONV_TICKS - 2 and rec["state"][-1, 0] == OPEN
    assert srec["reached"][-1, 0] == CONV_N and srec["last"][-1, 0] < CONV_TICKS, "the scenario does not converge inside the run"
    assert srec["last"][-1, 0] < rec["deadline"][-1, 0], "... nor inside the deadline"
    assert (rec["answered"][:, 0] <= srec["holds"][:, 0]).all() and rec["answered"][-1, 0] == CONV_N
    assert rec["t_all"][-1, 0] == srec["last"][-1, 0] and rec["t_first"][-1, 0] == srec["first"][-1, 0]
    o.close()


def test_origin_and_deadline_of_the_operations_are_the_images():
    """One route against another: the running-query section of the checkpoint image against the operations the model replays."""
    n = 97
    run = full_run(n)
    o, m = run["o"], run["m"]
    img = o.snapshot()
    qtab = tsn.words(img, tsn.sections(img), "qtab").reshape(256, 4)          # {id, origin, deadline, flags}
    hdr, rec = run["samples"]
    owners = 0
    for i, qid in enumerate(FULL_IDS):
        row = qtab[qid % 256]
        own = m.tables().owner(qid)
        assert (own is not None) == (row[0] == qid)
        if own:
            owners += 1
            assert (int(row[1]), int(row[2]), int(row[3])) == own[1:]
            assert (rec["origin"][-1, i], rec["deadline"][-1, i], rec["flags"][-1, i]) == own[1:]
    assert owners == 3


# ---- 5. qboard_summary on a hand-made sample array ----
def test_qboard_summary_on_a_hand_made_array():
    rec = np.zeros((6, 3), _ffi.QBOARD_ENTRY_DTYPE)
    rec["id"] = [11, 12, 13]
    a = rec[:, 0]                                                             # open from sample 1, closed at sample 4
    a["state"] = [WAITING, OPEN, OPEN, OPEN, CLOSED, CLOSED]
    a["deadline"][1:] = 40
    a["origin"][1:] = 2
    a["acks"] = [0, 3, 8, 9, 9, 9]
    a["responses"] = [0, 1, 2, 2, 2, 2]
    a["eligible"] = [0, 10, 10, 9, 9, 8]
    a["answered"] = [0, 3, 8, 8, 8, 7]
    a["silent"] = [0, 7, 2, 1, 1, 1]
    a["t_half"][2:] = 12
    a["t_90"][5:] = 0
    b = rec[:, 1]                                                             # open, displaced, then afresh and complete
    b["state"] = [OPEN, DISPLACED, OPEN, OPEN, OPEN, OPEN]
    b["deadline"] = [30, 30, 50, 50, 50, 50]
    b["acks"] = [2, 0, 1, 4, 4, 4]
    b["eligible"] = [4, 0, 4, 4, 4, 4]
    b["answered"] = [2, 0, 1, 4, 4, 4]
    for name, v in (("t_half", 19), ("t_90", 20), ("t_99", 20), ("t_all", 20)):
        b[name][3:] = v
    b["t_half"][:2] = 15
    s = _ffi.qboard_summary(rec, 16)
    assert s["id"].tolist() == [11, 12, 13] and s["state"].tolist() == [CLOSED, OPEN, WAITING]
    assert s[0].tolist() == (11, CLOSED, 24, 40, 9, 2, 8, 9, -12, -1, -1, -1, 1)[:8] + (12 - 24, -1, -1, -1, 1)
    assert s[1].tolist() == (12, OPEN, 34, 50, 4, 0, 4, 4, 19 - 34, 20 - 34, 20 - 34, 20 - 34, -1)
    assert s[2].tolist() == (13, WAITING) + (-1,) * 11
    assert len(_ffi.qboard_summary(np.zeros((0, 2), _ffi.QBOARD_ENTRY_DTYPE), 16)) == 2
    # and on a real run: every row is consistent with the samples it came from
    run = full_run(65)
    s = _ffi.qboard_summary(run["samples"][1], q_timeout(65))
    assert s["started"].tolist()[:4] == [q_timeout(65) + 5, 2, 3, 14] and s["state"].tolist() == [CLOSED, CLOSED, DISPLACED, CLOSED, WAITING]
    assert s["acks"][0] == run["samples"][1]["acks"][-1, 0] and s["silent_at_close"][1] >= 0 and s["to_half"][0] > 0 and s["to_all"][0] == -1


def test_the_rank_order_on_hand_made_records_with_ties():
    every = np.zeros(6, _ffi.QBOARD_NODE_DTYPE)
    every["id"] = np.arange(6)
    every["running"] = [1, 1, 0, 1, 1, 1]
    every["silent_ack"] = [2, 0, 9, 2, 3, 0]
    every["silent_resp"] = [0, 0, 1, 0, 0, 0]
    assert _ffi.qboard_rank(every, _ffi.QBOARD_BY_SILENT_ACK) == [4, 0, 3, 1, 5]
    assert _ffi.qboard_rank(every, _ffi.QBOARD_BY_SILENT_RESP, 3) == [0, 1, 3]


# ---- 6. the interface ----
def qboard_declared():
    src = re.sub(r"/\*.*?\*/", "", open(QBOARD_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t|const char\s*\*)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_qboard_header_declares_what_the_binding_binds():
    assert qboard_declared() == sorted("sim_" + s for s in _ffi.QBOARD_SYMBOLS)
    assert len(_ffi.QBOARD_SYMBOLS) == 9


def test_hip_library_exports_the_board():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in qboard_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    fn = dll.sim_qboard_version
    fn.restype = C.c_uint32
    assert fn() == 1
    assert lib.has_qboard and lib.qboard_version() == 1


def test_the_abi_and_the_nine_older_extensions_are_what_they_were(oracle):
    """The board is an extension: serf_sim.h, the nine older headers, their symbol lists and the ABI version do not know it; the
    oracle has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == tt.tsp.ABI_SYMBOLS_15
    assert tuple(_ffi.SPREAD_SYMBOLS) == tt.SPREAD_SYMBOLS_1 and tuple(_ffi.TRAFFIC_SYMBOLS) == tt.TRAFFIC_SYMBOLS_1
    assert tt.tree_declared() == sorted("sim_" + s for s in _ffi.TREE_SYMBOLS) and len(_ffi.TREE_SYMBOLS) == 9
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in tt.tsp.ABI_SYMBOLS_15)
    older = set(_ffi.ABI_SYMBOLS)
    for got in (_ffi.TRACK_SYMBOLS, _ffi.SERIES_SYMBOLS, _ffi.CENSUS_SYMBOLS, _ffi.ROLL_SYMBOLS, _ffi.LEDGER_SYMBOLS, _ffi.DETECT_SYMBOLS,
                _ffi.SPREAD_SYMBOLS, _ffi.TRAFFIC_SYMBOLS, _ffi.TREE_SYMBOLS):
        older |= set(got)
    assert not set(_ffi.QBOARD_SYMBOLS) & older
    lib = serf_amd.load()
    assert lib.abi_version() == 15 and oracle.abi_version() == 15 and lib.tree_version() == 1
    assert not oracle.has_qboard and oracle.qboard_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.QBOARD_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)
    o = _ffi.Sim(oracle, _ffi.make_config(64))
    for call in (lambda: o.qboard_start([1]), o.qboard_count, o.qboard_read, o.qboard_stop, lambda: o.qboard_now([1]), lambda: o.qboard_silent(0),
                 o.qboard_nodes, o.qboard_top):
        with pytest.raises(NotImplementedError):
            call()
    o.close()


def test_qboard_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include "serf_sim_qboard.h"\n'
                    'int main(void){printf("%zu %u %u %u %u %u %u %u %u %u %u %u %u %u\\n",sizeof(sim_qboard_node),SIM_QBOARD_MAX,'
                    "SIM_QBOARD_MAX_SAMPLES,SIM_QBOARD_VERSION,SIM_QBOARD_HEADER_WORDS,SIM_QBOARD_ENTRY_WORDS,SIM_QBOARD_TOP_MAX,SIM_QBOARD_NODE_WORDS,"
                    "SIM_QBOARD_WAITING,SIM_QBOARD_OPEN,SIM_QBOARD_CLOSED,SIM_QBOARD_DISPLACED,SIM_QBOARD_BY_SILENT_ACK,SIM_QBOARD_BY_SILENT_RESP);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [_ffi.QBOARD_NODE_DTYPE.itemsize, _ffi.QBOARD_MAX, _ffi.QBOARD_MAX_SAMPLES, 1, _ffi.QBOARD_HEADER_WORDS, _ffi.QBOARD_ENTRY_WORDS,
                   _ffi.QBOARD_TOP_MAX, _ffi.QBOARD_NODE_WORDS, WAITING, OPEN, CLOSED, DISPLACED, _ffi.QBOARD_BY_SILENT_ACK, _ffi.QBOARD_BY_SILENT_RESP]
    assert got[:2] == [64, 64] and (HW, EW) == (8, 16)
    off = {n: _ffi.QBOARD_HEADER_DTYPE.fields[n][1] // 8 for n in _ffi.QBOARD_HEADER_DTYPE.names}
    assert off == dict(tick=0, running=1, n=2, open=3, closed=4, waiting=5, displaced=6, new=7)
    off = {n: _ffi.QBOARD_ENTRY_DTYPE.fields[n][1] / 8 for n in _ffi.QBOARD_ENTRY_DTYPE.names}
    assert off == dict(id=0, state=0.5, origin=1, flags=1.5, deadline=2, acks=3, responses=4, eligible=5, answered=6, responded=7, silent=8,
                       new_acks=9, new_responses=10, t_first=11, t_half=12, t_90=13, t_99=14, t_all=15)
    off = {n: _ffi.QBOARD_NODE_DTYPE.fields[n][1] / 8 for n in _ffi.QBOARD_NODE_DTYPE.names}
    assert off == dict(id=0, running=0.5, asked=1, acked=2, responded=3, silent_ack=4, silent_resp=5, reserved=6)
    for n in (1, 5, 64):
        hdr, rec = _ffi.qboard_split(np.arange(3 * (8 + 16 * n), dtype=np.uint64), n)
        assert hdr.shape == (3,) and rec.shape == (3, n) and rec["t_all"][1, n - 1] == 2 * (8 + 16 * n) - 1


def test_the_cap_is_the_sources():
    """QBOARD_GRID above mirrors these lines; a change there has to move the second-pass size of tests/test_qboard_gpu.py."""
    src = open(QBOARD_INC).read()
    assert re.search(r"^#define QBOARD_GRID %du\b" % QBOARD_GRID, src, re.M)
    assert src.count("const size_t per_pass = (size_t)gridDim.x * BLOCK;") == 1
    assert "p.G = qboard_grid(h);" in src and "std::min<size_t>(((size_t)h->d.Nl + BLOCK - 1) / BLOCK, QBOARD_GRID)" in src
    assert "query_should_process(" in src and "static bool query_should_process" not in src, "the board calls the tick's function, it has no copy"
    assert re.search(r"^#define BLOCK %d$" % BLOCK, open(os.path.join(ROOT, "serf_amd", "csrc", "serf_sim.hip")).read(), re.M)
    assert q_timeout(SECOND_N) == 96 and q_timeout(97) == 32 and q_timeout(257) == 48
