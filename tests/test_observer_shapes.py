"""The observers — trackers, series, census, sim_convergence(_many) — at cluster sizes that are ragged, tiny, idle, or beyond what
one pass of a kernel's grid covers: the part that needs no GPU.  This file owns the scenarios and the conditions that make them
non-trivial; it runs them on the CPU oracle with the reference models (tests/track_model.py, series_model.py, census_model.py).
tests/test_observer_shapes_gpu.py drives the HIP library through the same scripts and compares word for word.

The observer kernels share one shape: a pass loop in which whole waves stay together (lanes past the last node kept alive for
the ballots), ballots into wave-uniform or LDS counters, a column of partial results per workgroup, a second kernel that folds
the rows.  What each size is there to catch:

  ragged(n)     1, 2, 3    one lane with a node; fewer other nodes than the fan-out.  A kernel that counts lanes >= Nl reports
                           `running` / `last_up` / `up` of 64 or 256 instead of 1 .. 3.
                63, 64, 65 a wave short by one, a whole wave, a whole wave plus one lane.  63 and 65 catch a kernel that counts
                           lanes >= Nl (64 is their control: there it cannot show).  65 catches one that drops the last partial
                           wave's ballot: that wave's only lane is node 64, the one that crashes and the subject of three trackers
                           — before tick 4 `running` would read 64, and the JOIN about it 64 of 65.
                127        two waves, the second short by one: both of the above with a whole wave in front.
                257        a second workgroup of ONE lane for the series and convergence kernels (256 nodes a workgroup): that lane
                           is the crashed node; a dropped ballot or a grid one workgroup short leaves it counted as running / never
                           counts what it holds.
                1000       the ragged size the rest of the suite uses.
                1025       a second workgroup of one lane for the tracker kernel (256 lanes x 4 nodes a workgroup).
  nobody_runs   1, 3, 65   every node crashed: `if (!nup) continue`, `if (up)`, and the fold that turns the ~0 a min word starts
                           from into 0 — a kernel that leaves ~0 there fails on the six clock words and n_known_min.
  second pass   cap + 65   one whole wave and one lane in pass 1 of a pass loop.  The crashed node and the event's origin lie in
                           that pass: a loop that stops one pass early counts the crashed node as running (it reads nothing of
                           it) and misses the nodes of the second pass that hold the event.

Everything compared is an exact integer."""
import functools
import os
import re

import numpy as np
import pytest

from serf_amd import _ffi
from tests._oracle import load_oracle
from tests.census_model import CensusModel
from tests.series_model import SeriesModel, as_records
from tests.test_track_gpu import BIJECTION, FAILED, KRANDOM, SUSPECT_OR_DEAD
from tests.track_model import TrackModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "serf_amd", "csrc")
NEVER, NOSLOT = _ffi.TRACK_NEVER, 0xFFFFFFFF
KW = dict(fanout=4, event_ring=64, query_ring=64, probe_interval=5, loss=0.01, ring_overflow=4, join_sync=True)
FANOUTS = {"krandomnodes": KRANDOM, "bijection": BIJECTION}
EVENT_KEY, QUERY_ID = 0x77, 777

# nodes one pass of a kernel's grid covers (a pass loop's second turn needs more).  If one of these changes in the source,
# test_the_caps_are_the_sources says so and the second-pass sizes below move with it.
BLOCK = 256                                  # serf_sim.hip: #define BLOCK 256
SER_CAP = 1024 * BLOCK                       # serf_sim_series.inc: #define SER_GRID 1024u; per_pass = gridDim.x * BLOCK
TRK_CAP = 1024 * BLOCK * 4                   # serf_sim_track.inc: #define TRK_GRID 1024u, TRK_NPL 4; per_pass = gridDim.x * BLOCK * TRK_NPL
CONV_CAP = 8192 * BLOCK                      # serf_sim_host.inc grid_for: min((n + BLOCK - 1) / BLOCK, 8192) workgroups
SECOND_PASS = 65                             # nodes of the second pass: one whole wave and one lane

RAGGED_SIZES = (1, 2, 3, 63, 64, 65, 127, 257, 1000, 1025)
RAGGED_TICKS = 90
CENSUS_SUBJECTS = 8
# measured on the oracle, both fan-out models: size -> (suspicion first, all, failed first, all, event all)
RAGGED_FIGURES = {65: (6, 10, 42, 46, (5,)), 1000: (9, 15, 69, 74, (7, 8))}


# 63 nodes run under the next seed.  Under the default one, with kRandomNodes, node 24 never hears of node 61's leave (loss 0.01,
# the intent's retransmissions run out at tick 15 with 61 of 62 holding it, there is no push-pull): the LEAVE tracker cannot latch
# `all` however long the run — 400 ticks tried — and "every tracker latches `all`" is a condition of the scenario.  Seeds + 1, + 3,
# + 4 and + 5 meet every condition with both fan-out models (+ 2 does not); every other size meets them under the default seed.
RAGGED_SEED = {63: _ffi.DEFAULT_SEED + 1}


def ragged_kw(n, fan):
    return dict(KW, view_slots=0 if n <= 65 else 16, flags=FANOUTS[fan], seed=RAGGED_SEED.get(n, _ffi.DEFAULT_SEED))


def ragged_script(sim, n, add, step, ticks=RAGGED_TICKS):
    """The same script for both sides.  add(spec) registers one tracker, step(k) advances k ticks: the model side one tick at a
    time, the HIP side in two calls (10 and ticks - 10).  Returns ({name: tracker handle}, {name: (kind, key, ltime)})."""
    last, hs, ru = n - 1, {}, {}
    if n > 1:
        sim.inject(4, _ffi.OP_CRASH, last)              # the node of the partial wave
        hs["suspicion"] = add(_ffi.member_tracker(last, FAILED, SUSPECT_OR_DEAD, start=4))   # "suspected or worse"
        hs["failed"] = add(_ffi.member_tracker(last, FAILED, start=4))                        # "declared failed"
    ru["event"] = (_ffi.K_EVENT, EVENT_KEY, sim.stats(0).event_time)
    ru["join"] = (_ffi.K_JOIN, last, 1)
    hs["event"] = add(_ffi.rumour_tracker(*ru["event"]))
    hs["join"] = add(_ffi.rumour_tracker(*ru["join"]))
    sim.user_event(0, EVENT_KEY, 64)
    step(10)
    if n > 2:
        ru["leave"] = (_ffi.K_LEAVE, n - 2, sim.stats(n - 2).member_time)
        hs["leave"] = add(_ffi.rumour_tracker(*ru["leave"]))
        sim.leave(n - 2)
    ru["query"] = (_ffi.K_QUERY, QUERY_ID, sim.stats(0).query_time)
    hs["query"] = add(_ffi.rumour_tracker(*ru["query"]))
    sim.query(0, QUERY_ID, _ffi.F_ACK)
    step(ticks - 10)
    return hs, ru


def five_rumours(ru, n):
    """The scenario's rumours as sim_convergence names them: the event, the query, the JOIN every baseline holds, the LEAVE, and a
    JOIN at the LEAVE's Lamport time (a view entry answers for both kinds); without a leave (n <= 2) two that nobody holds."""
    leave = ru.get("leave", (_ffi.K_LEAVE, 0, 2))
    return [ru["event"], ru["query"], ru["join"], leave, (_ffi.K_JOIN, leave[1], leave[2])]


def answers(sim, n, ru, noslot=None):
    """Everything the scenario reads at the end besides the observers' buffers, from either library."""
    five = five_rumours(ru, n)
    lt = ru["event"][2]            # the event's own Lamport time: its bucket is neither empty nor full on most nodes
    out = dict(digest=sim.digest(), cluster_stats=sim.cluster_stats(), query_status=sim.query_status(QUERY_ID),
               acks=sim.query_responders(QUERY_ID, 0), responses=sim.query_responders(QUERY_ID, 1))
    for obs in sorted({0, n - 1}):
        st, ltm = sim.members(obs)
        s = sim.stats(obs)
        out[f"members({obs})"] = (st.tolist(), ltm.tolist())
        out[f"stats({obs})"] = {f: int(getattr(s, f)) for f, _ in _ffi.Stats._fields_}
    out["convergence"] = [sim.convergence(*r) for r in five]
    out["convergence_many"] = sim.convergence_many(five)
    # key 0 of an EVENT / QUERY names no rumour (include/serf_sim.h): seen == 0, up == the running nodes, in both entry points
    out["key 0"] = [sim.convergence(_ffi.K_EVENT, 0, lt), sim.convergence(_ffi.K_QUERY, 0, lt)]
    out["key 0 mixed"] = sim.convergence_many([five[0], (_ffi.K_EVENT, 0, lt), five[1], (_ffi.K_QUERY, 0, lt)] + five[2:] + [(_ffi.K_EVENT, 0, lt)])
    if noslot is not None:         # a subject that never got a view slot: the baseline entry answers
        asked = [(k, noslot, t) for k in (_ffi.K_JOIN, _ffi.K_LEAVE) for t in (1, 2)]
        out["no slot"] = [sim.convergence(*r) for r in asked] + [sim.convergence_many(asked)]
    return out


def check_key0(ans, five_seen):
    up = ans["cluster_stats"]["up"]
    assert ans["key 0"] == [(0, up), (0, up)]
    seen, many_up = ans["key 0 mixed"]
    assert many_up == up and seen == [five_seen[0], 0, five_seen[1], 0] + five_seen[2:] + [0]


@functools.lru_cache(maxsize=None)
def ragged_oracle(n, fan):
    """ragged(n) on the oracle with the three models chained, once per session.  Nobody changes what it returns:
    dict(o, trackers {name: result}, rumours, series [samples][64], census (headers, records), answers, noslot)."""
    o = _ffi.Sim(load_oracle(), _ffi.make_config(n, **ragged_kw(n, fan)))
    tm, cm = TrackModel(o), CensusModel(o)
    sm = SeriesModel(o, lambda: (tm.evaluate(), cm.after_tick(o.tick - 1)))
    sm.start(0, 1, RAGGED_TICKS)
    cm.start(0, 1, RAGGED_TICKS, CENSUS_SUBJECTS)
    hs, ru = ragged_script(o, n, tm.add, sm.step)
    noslot = None
    if ragged_kw(n, fan)["view_slots"]:
        free = np.nonzero(o.dump(_ffi.ARR_SLOTMAP) == NOSLOT)[0]
        free = free[(free != 0) & (free != n - 1)]
        assert len(free), "no subject without a view slot"
        noslot = int(free[len(free) // 2])
    return dict(o=o, trackers={k: tm.result(h) for k, h in hs.items()}, rumours=ru, series=sm.read(), census=cm.read(),
                answers=answers(o, n, ru, noslot), noslot=noslot)


def check_ragged(n, run):
    """ragged(n) does what it is for (otherwise equal words would show little)."""
    cs, trk, rec = run["answers"]["cluster_stats"], run["trackers"], as_records(run["series"])
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0          # the run stays inside the model's bounds
    assert len(rec) == RAGGED_TICKS and run["census"][0]["tick"].tolist() == list(range(1, RAGGED_TICKS + 1))
    if n >= 3:
        assert len(trk) == 6
        for name, r in trk.items():
            assert r["all"] != NEVER and r["all"] < RAGGED_TICKS and r["state"] == 2, (name, r)
    if n >= 63:
        for name in ("suspicion", "failed", "event", "leave", "query"):
            assert trk[name]["first"] < trk[name]["all"], (name, trk[name])
    assert rec["timers"].max() >= n - 1
    running = rec["running"].tolist()
    want = [n] + ([n - 1] if n > 1 else []) + ([n - 2] if n > 2 else [])
    assert [x for i, x in enumerate(running) if not i or running[i - 1] != x] == want, "running: n, then n - 1, then n - 2"
    assert cs["up"] == want[-1]
    if n in RAGGED_FIGURES:
        s1, sa, f1, fa, ea = RAGGED_FIGURES[n]
        assert (trk["suspicion"]["first"], trk["suspicion"]["all"], trk["failed"]["first"], trk["failed"]["all"]) == (s1, sa, f1, fa)
        assert trk["event"]["all"] in ea
    if n > 65:
        assert run["noslot"] is not None and run["answers"]["no slot"][0] == (cs["up"], cs["up"]) and run["answers"]["no slot"][1] == (0, cs["up"])
    conv = run["answers"]["convergence"]
    assert run["answers"]["convergence_many"] == ([s for s, _ in conv], cs["up"]) and all(u == cs["up"] for _, u in conv)
    check_key0(run["answers"], [s for s, _ in conv])


@pytest.mark.parametrize("fan", sorted(FANOUTS))
@pytest.mark.parametrize("n", RAGGED_SIZES)
def test_ragged_is_nontrivial_on_the_oracle(n, fan):
    """Every listed size: the reference stays inside its bounds and the scenario moves every observer (check_ragged); key 0 of
    an EVENT / QUERY is held by nobody — the oracle against the literal (0, up), tests/third_model.py has no convergence."""
    check_ragged(n, ragged_oracle(n, fan))


# ---- nobody runs ----
IDLE_SIZES, IDLE_TICKS, IDLE_CRASH = (1, 3, 65), 12, 5


def idle_script(sim, n, add, step):
    for x in range(n):
        sim.inject(IDLE_CRASH, _ffi.OP_CRASH, x)
    hs = dict(member=add(_ffi.member_tracker(0, 1 << _ffi.STATUS_ALIVE)), event=add(_ffi.rumour_tracker(_ffi.K_EVENT, EVENT_KEY, 99)),
              join=add(_ffi.rumour_tracker(_ffi.K_JOIN, 0, 99)))
    step(IDLE_TICKS)
    return hs


def idle_answers(sim):
    return dict(digest=sim.digest(), cluster_stats=sim.cluster_stats(), convergence=sim.convergence(_ffi.K_EVENT, EVENT_KEY, 99),
                convergence_many=sim.convergence_many([(_ffi.K_JOIN, 0, 1), (_ffi.K_EVENT, EVENT_KEY, 99), (_ffi.K_EVENT, 0, 99)]))


@functools.lru_cache(maxsize=None)
def idle_oracle(n, fan):
    o = _ffi.Sim(load_oracle(), _ffi.make_config(n, **dict(KW, view_slots=0, flags=FANOUTS[fan])))
    tm, cm = TrackModel(o), CensusModel(o)
    sm = SeriesModel(o, lambda: (tm.evaluate(), cm.after_tick(o.tick - 1)))
    sm.start(0, 1, IDLE_TICKS)
    cm.start(0, 1, IDLE_TICKS, CENSUS_SUBJECTS)
    hs = idle_script(o, n, tm.add, sm.step)
    return dict(o=o, trackers={k: tm.result(h) for k, h in hs.items()}, series=sm.read(), census=cm.read(), answers=idle_answers(o))


def check_idle(n, run):
    rec, trk, ans = as_records(run["series"]), run["trackers"], run["answers"]
    assert rec["running"].tolist() == [n] * IDLE_CRASH + [0] * (IDLE_TICKS - IDLE_CRASH)
    for f in ("clock_min", "clock_max", "event_clock_min", "event_clock_max", "query_clock_min", "query_clock_max", "n_known_min", "n_known_max"):
        assert (rec[f][:IDLE_CRASH] > 0).all() and (rec[f][IDLE_CRASH:] == 0).all(), f      # 0, not the ~0 a min starts from
    assert trk["member"]["all"] == 1 and trk["member"]["state"] == 2 and trk["member"]["evaluated"] == 1
    for name in ("event", "join"):
        r = trk[name]
        assert (r["evaluated"], r["last_up"], r["first"], r["state"], r["peak"]) == (IDLE_TICKS, 0, NEVER, 1, 0), (name, r)
    assert ans["convergence"] == (0, 0) and ans["convergence_many"] == ([0, 0, 0], 0) and ans["cluster_stats"]["up"] == 0
    hdr = run["census"][0]
    assert hdr["running"].tolist() == rec["running"].tolist()


@pytest.mark.parametrize("fan", sorted(FANOUTS))
@pytest.mark.parametrize("n", IDLE_SIZES)
def test_nobody_runs_on_the_oracle(n, fan):
    check_idle(n, idle_oracle(n, fan))


# ---- the second pass of the three pass loops ----
BIG_KW = dict(KW, view_slots=16, flags=KRANDOM)
SERIES_N, SERIES_TICKS, SERIES_PERIOD = SER_CAP + SECOND_PASS, 9, 4
TRACK_N, TRACK_TICKS, TRACK_WINDOW = TRK_CAP + SECOND_PASS, 14, (10, 4)     # (start, max_age): evaluated after ticks 10 .. 13
CONV_N, CONV_TICKS = CONV_CAP + SECOND_PASS, 9


def big_start(sim, n):
    """The crashed node and the event's origin both lie in the second pass.  Returns the event as sim_convergence names it."""
    sim.inject(2, _ffi.OP_CRASH, n - 1)
    ev = (_ffi.K_EVENT, EVENT_KEY, sim.stats(n - 3).event_time)
    sim.user_event(n - 3, EVENT_KEY, 64)
    return ev


@functools.lru_cache(maxsize=None)
def series_second_pass_oracle():
    n = SERIES_N
    o = _ffi.Sim(load_oracle(), _ffi.make_config(n, **BIG_KW))
    sm = SeriesModel(o)
    sm.start(0, SERIES_PERIOD, 100)
    big_start(o, n)
    sm.step(SERIES_TICKS)
    return o, sm.read()


def check_series_second_pass(words):
    rec = as_records(words)
    assert rec["tick"].tolist() == [1, 5, 9]
    assert rec["running"].tolist() == [SERIES_N, SERIES_N - 1, SERIES_N - 1]           # the crashed node, of the second pass
    assert rec["timers"][-1] > 0 and rec["records"][-1, _ffi.K_EVENT - 1] > 0
    assert rec["records"][:, _ffi.K_EVENT - 1].tolist()[0] == 4                        # the origin's first four packets


def test_series_second_pass_on_the_oracle():
    assert SERIES_N == 262209
    o, words = series_second_pass_oracle()
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    check_series_second_pass(words)


def track_second_pass_script(sim, n, add, step):
    start, age = TRACK_WINDOW
    ev = big_start(sim, n)
    hs = dict(suspicion=add(_ffi.member_tracker(n - 1, FAILED, SUSPECT_OR_DEAD, start=start, max_age=age)),
              event=add(_ffi.rumour_tracker(*ev)), join=add(_ffi.rumour_tracker(_ffi.K_JOIN, n - 1, 1, start=start, max_age=age)))
    step(TRACK_TICKS)
    return hs


@functools.lru_cache(maxsize=None)
def track_second_pass_oracle():
    n = TRACK_N
    o = _ffi.Sim(load_oracle(), _ffi.make_config(n, **BIG_KW))
    tm = TrackModel(o)
    hs = track_second_pass_script(o, n, tm.add, tm.step)
    return o, {k: tm.result(h) for k, h in hs.items()}


def check_track_second_pass(trk):
    ev, su, jo = trk["event"], trk["suspicion"], trk["join"]
    assert ev["first"] == 1 and ev["all"] != NEVER and ev["evaluated"] == ev["all"] and ev["last_up"] == TRACK_N - 1
    assert su["evaluated"] == TRACK_WINDOW[1] and su["state"] == 2 and su["all"] == NEVER
    assert 0 < su["last"] < su["last_up"] == TRACK_N - 1                                 # half way: what discriminates
    assert jo["all"] == TRACK_WINDOW[0] + 1 and jo["last"] == jo["last_up"] == TRACK_N - 1


def test_trackers_second_pass_on_the_oracle():
    assert TRACK_N == 1048641
    o, trk = track_second_pass_oracle()
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    check_track_second_pass(trk)


def conv_second_pass_asked(n, ev):
    """64 entries: the event three times over, an event key and a query nobody sent, JOIN and LEAVE about three subjects at
    Lamport times 1 (every baseline holds it) and 2 (nobody does), over and over."""
    some = [ev, ev, ev, (_ffi.K_EVENT, EVENT_KEY + 1, ev[2]), (_ffi.K_QUERY, QUERY_ID, 1)]
    some += [(k, s, t) for k in (_ffi.K_JOIN, _ffi.K_LEAVE) for s in (0, n // 2, n - 1) for t in (1, 2)]
    return [some[i % len(some)] for i in range(64)]


def conv_second_pass_answers(sim, n, ev):
    return dict(event=sim.convergence(*ev), join=sim.convergence(_ffi.K_JOIN, n - 1, 1), many=sim.convergence_many(conv_second_pass_asked(n, ev)),
                cluster_stats=sim.cluster_stats(), digest=sim.digest())


@functools.lru_cache(maxsize=None)
def conv_second_pass_oracle():
    n = CONV_N
    o = _ffi.Sim(load_oracle(), _ffi.make_config(n, **BIG_KW))
    ev = big_start(o, n)
    o.step(CONV_TICKS)
    return o, ev, conv_second_pass_answers(o, n, ev)


def check_conv_second_pass(ans):
    seen, up = ans["event"]
    assert up == CONV_N - 1 == ans["cluster_stats"]["up"] and 0 < seen < up            # half way: what discriminates
    assert ans["join"] == (up, up)
    many, many_up = ans["many"]
    assert many_up == up and many[:5] == [seen, seen, seen, 0, 0] and many[5:17] == [up, 0] * 6 and many[17:22] == many[:5]


def test_convergence_second_pass_on_the_oracle():
    assert CONV_N == 2097217
    o, ev, ans = conv_second_pass_oracle()
    assert ans["cluster_stats"]["overflow"] == 0 and ans["cluster_stats"]["ops_dropped"] == 0
    check_conv_second_pass(ans)


def test_the_caps_are_the_sources():
    """The three caps above mirror these lines; a change there has to move the second-pass sizes."""
    def src(name):
        return open(os.path.join(CSRC, name)).read()
    assert re.search(r"^#define BLOCK 256$", src("serf_sim.hip"), re.M)
    assert re.search(r"^#define SER_GRID 1024u\b", src("serf_sim_series.inc"), re.M)
    assert "const size_t per_pass = (size_t)gridDim.x * BLOCK;" in src("serf_sim_series.inc")
    assert re.search(r"^#define TRK_GRID 1024u\b", src("serf_sim_track.inc"), re.M) and re.search(r"^#define TRK_NPL 4\b", src("serf_sim_track.inc"), re.M)
    assert "const size_t per_pass = (size_t)gridDim.x * BLOCK * TRK_NPL;" in src("serf_sim_track.inc")
    assert "static inline int grid_for(size_t n) { return (int)std::min<size_t>((n + BLOCK - 1) / BLOCK, 8192); }" in src("serf_sim_host.inc")
    assert "convergence_many_kernel<<<grid_for(h->d.Nl), BLOCK, 0, s>>>" in src("serf_sim_api.inc")
