"""Member gazette (include/serf_sim_gazette.h), the part that needs no GPU: the extension's interface next to the ABI and the other
eleven extensions, the reference model's invariants (tests/gazette_model.py), the model against an independent route on the
oracle — the event log of a run with every node watched —, and the conditions of the scenarios that tests/test_gazette_gpu.py
runs on the GPU as well.

This file owns those scenarios.  A scenario is (nodes, configuration, a script drive(sim, step), the gazette's start arguments);
run() is the script on a fresh oracle with a GazetteModel behind the ticks, once per session.

  main       tests/test_series.py's scenario at 1 000 nodes — six crashes, a leave — with a Reaper that reaps (reap_interval
             10, tombstone_timeout 60: the second leaver goes), a force-leave with prune of the first leaver once it is
             Left (one Reap a node: about a Failed member it is Leave and Reap in ONE tick, which a diff sees as their net
             transition and the comparison with the event log would have to exclude), and two crash-revive pairs: the node
             that crashed first is revived 16 ticks after the cluster declared it Failed (inside flap_window = 60), the
             second at tick 230, about 150 ticks after (outside)
  ragged     the ragged script of tests/test_observer_shapes.py at 3, 64, 65 (dense views: view_slots == n_nodes) and 257 nodes
  vshards    64 nodes as four virtual shards on one handle
  idle       every node crashes in one tick: nobody runs
  second     GAZETTE_GRID x BLOCK + 65 nodes, 20 ticks, two crashes: the pass loop runs twice
  recycle    257 nodes, 4 view slots recycled every 20 ticks under churn: a slot goes to ANOTHER subject between two samples
  boundary   257 nodes; 255 and 256 crash in one tick: two rows of the subject map that tie across a workgroup boundary
  groups     main's first 100 ticks with 200 view slots: a shadow group holds four slots, the high-water mark crosses groups

Everything compared is an exact integer."""
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
from tests import test_ledger as tl
from tests import test_observer_shapes as shapes
from tests import test_recycle
from tests.gazette_model import GazetteModel, classify, state, state_of
from tests.test_track import ABI_SYMBOLS_15
from tests.test_track_gpu import BIJECTION, KRANDOM, KW, script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "serf_sim_gazette.h")
INC = os.path.join(ROOT, "serf_amd", "csrc", "serf_sim_gazette.inc")
BLOCK = 256                                    # serf_sim.hip: #define BLOCK 256
COLS = _ffi.GAZETTE_COLUMNS
OTHERS = ("TRACK", "SERIES", "CENSUS", "ROLL", "LEDGER", "DETECT", "SPREAD", "TRAFFIC", "TREE", "QBOARD", "CATALOG")


def gazette_grid():
    """serf_sim_gazette.inc: #define GAZETTE_GRID — workgroups of the scan kernel at most; per pass GAZETTE_GRID x BLOCK nodes."""
    return int(re.search(r"#define GAZETTE_GRID (\d+)u", open(INC).read()).group(1))


# ---- scenarios ----
N, TICKS, WINDOW = 1000, 260, 60
MAIN_KW = dict(KW, reap_interval=10, tombstone_timeout=60, reconnect_timeout=100000, push_pull_interval=20, join_sync=False)
REVIVE_NEAR, REVIVE_FAR, PRUNE_AT, LEAVE_AT, LEAVE_DELAY = 16, 200, 110, 60, 30


def failed_at(n, kw, subject, crash_tick):
    """A dry run on the oracle: the first tick behind which every running node holds `subject` Failed."""
    o = tl.maker(n, kw)()
    o.inject(crash_tick, _ffi.OP_CRASH, subject)
    for _ in range(400):
        o.step(1)
        bits, slot_of, up = state(o)
        if slot_of[subject] != 0xFFFFFFFF and (state_of(bits[slot_of[subject]][up]) == _ffi.STATUS_FAILED).all():
            t = o.tick - 1
            o.close()
            return t
    raise AssertionError("never declared Failed")


def main_drive(ticks=TICKS):
    def drive(sim, step):
        s = script(N)
        for t, c in zip(s["crash_at"], s["crashed"]):
            sim.inject(t, _ffi.OP_CRASH, c)
        for t, x in ((MAIN_NEAR_TICK(), s["crashed"][0]), (REVIVE_FAR, s["crashed"][1])):     # a restarted process joins again
            sim.inject(t, _ffi.OP_REVIVE, x)
            sim.inject(t + 1, _ffi.OP_JOIN, x, s["live"][2])
        for t, x in ((LEAVE_AT, s["live"][0]), (LEAVE_AT + 10, s["live"][3])):          # (what sim_leave injects)
            sim.inject(t, _ffi.OP_LEAVE, x)
            sim.inject(t + LEAVE_DELAY + 1, _ffi.OP_LEAVE_FINISH, x)
            sim.inject(t + 2 * LEAVE_DELAY + 2, _ffi.OP_CRASH, x)
        sim.inject(PRUNE_AT, _ffi.OP_FORCE_LEAVE, s["live"][1], s["live"][0], 1)        # the first leaver is Left by then: erased at once
        for te, node, key in s["events"][:10]:
            sim.inject(te, _ffi.OP_USER_EVENT, node, key, 64)
        step(ticks)
    return drive


@functools.lru_cache(maxsize=None)
def MAIN_NEAR_TICK():
    """The tick of the near revive: REVIVE_NEAR ticks after everybody holds the first crashed node Failed (plain run, krandomnodes)."""
    s = script(N)
    return failed_at(N, dict(MAIN_KW, flags=KRANDOM), s["crashed"][0], s["crash_at"][0]) + REVIVE_NEAR


def churn_drive(n, ticks):
    def drive(sim, step):
        for op in test_recycle.churn_ops(n, 34, every=6, down=4, start=2):      # (a crash in every tick that recycles: 20, 80, 140, 200)
            sim.inject(*op)
        step(ticks)
    return drive


def crashes_drive(ticks, crashes):
    def drive(sim, step):
        for t, x in crashes:
            sim.inject(t, _ffi.OP_CRASH, x)
        step(ticks)
    return drive


RECYCLE_N, RECYCLE_TICKS = 257, 220
RECYCLE_KW = dict(test_recycle.KW, view_slots=4, recycle_interval=20, flags=KRANDOM)
SECOND_TICKS = 20
BOUNDARY_TICKS = 120


def second_n():
    return gazette_grid() * BLOCK + shapes.SECOND_PASS


def scenario(name, arg=None):
    """(nodes, configuration, drive, the gazette's start arguments)."""
    start = dict(first_tick=0, period=1, capacity=1 << 10, flap_window=WINDOW)
    if name == "main":                                           # arg: (fan-out model, period[, flap_window])
        return N, dict(MAIN_KW, flags=shapes.FANOUTS[arg[0]]), main_drive(), dict(start, period=arg[1], flap_window=arg[2] if len(arg) > 2 else WINDOW)
    if name == "groups":
        return N, dict(MAIN_KW, view_slots=200, flags=KRANDOM), main_drive(100), start
    if name == "ragged":                                         # arg: nodes
        return arg, shapes.ragged_kw(arg, "krandomnodes"), lambda sim, step: shapes.ragged_script(sim, arg, lambda spec: None, step), start
    if name == "vshards":
        return 64, dict(shapes.ragged_kw(64, "bijection"), vshards=4), lambda sim, step: shapes.ragged_script(sim, 64, lambda spec: None, step), start
    if name == "idle":
        return 64, dict(shapes.KW, view_slots=0, flags=KRANDOM), lambda sim, step: shapes.idle_script(sim, 64, lambda spec: None, step), start
    if name == "second":
        n = second_n()
        return n, shapes.BIG_KW, crashes_drive(SECOND_TICKS, [(2, n - 1), (3, 5)]), dict(start, period=5)
    if name == "boundary":
        return 257, dict(shapes.KW, view_slots=16, flags=KRANDOM), crashes_drive(BOUNDARY_TICKS, [(2, 255), (2, 256)]), start
    if name == "recycle":                                        # arg: period
        return RECYCLE_N, RECYCLE_KW, churn_drive(RECYCLE_N, RECYCLE_TICKS), dict(start, period=arg)
    raise KeyError(name)


def tops(m, ks=(1, 10, 64)):
    return {(which, col, k): m.top(which, col, k) for which in (0, 1) for col in range(8) for k in ks}


@functools.lru_cache(maxsize=None)
def run(name, arg=None):
    """Once per session; nobody changes what it returns: dict(o, m, samples, nodes, subjects, count)."""
    n, kw, drive, start = scenario(name, arg)
    o = tl.maker(n, kw)()
    m = GazetteModel(o)
    m.start(**start)
    drive(o, m.step)
    return dict(o=o, m=m, samples=m.read(), nodes=m.nodes.copy(), subjects=m.subj.copy(), count=m.count())


# ---- 1. the interface ----
def declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t)\s+(sim_[a-z_0-9]+)\s*\(", src)))


def test_header_declares_what_the_binding_binds():
    assert declared() == sorted("sim_" + s for s in _ffi.GAZETTE_SYMBOLS)
    assert len(_ffi.GAZETTE_SYMBOLS) == 8


def test_hip_library_exports_the_gazette():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    assert lib.has_gazette and lib.gazette_version() == 1


def test_the_abi_and_the_other_extensions_are_what_they_were(oracle):
    """The gazette is an extension: serf_sim.h, the other eleven symbol tables and the ABI version do not know it; the oracle
    has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == ABI_SYMBOLS_15
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in ABI_SYMBOLS_15)
    mine = set(_ffi.GAZETTE_SYMBOLS)
    assert not mine & set(_ffi.ABI_SYMBOLS)
    for other in OTHERS:
        assert not mine & set(getattr(_ffi, other + "_SYMBOLS")), other
    lib = serf_amd.load()
    assert lib.abi_version() == 15 and oracle.abi_version() == 15
    assert [getattr(lib, g.lower() + "_version")() for g in OTHERS] == [1] * len(OTHERS)
    assert not oracle.has_gazette and oracle.gazette_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.GAZETTE_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)
    with pytest.raises(NotImplementedError):
        _ffi.Sim(oracle, _ffi.make_config(64)).gazette_start()


def test_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include "serf_sim_gazette.h"\n'
                    'int main(void){printf("%zu %zu %zu %u %u %u %u %u\\n",sizeof(sim_gazette_sample),sizeof(sim_gazette_row),'
                    "sizeof(sim_gazette_rank),SIM_GAZETTE_WORDS,SIM_GAZETTE_COLS,SIM_GAZETTE_TOP_MAX,SIM_GAZETTE_MAX_SAMPLES,"
                    "SIM_GAZETTE_VERSION);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [_ffi.GAZETTE_SAMPLE_DTYPE.itemsize, 4 * _ffi.GAZETTE_COLS, _ffi.GAZETTE_RANK_DTYPE.itemsize, _ffi.GAZETTE_WORDS,
                   _ffi.GAZETTE_COLS, _ffi.GAZETTE_TOP_MAX, _ffi.GAZETTE_MAX_SAMPLES, 1]
    off = {n: _ffi.GAZETTE_SAMPLE_DTYPE.fields[n][1] // 8 for n in _ffi.GAZETTE_SAMPLE_DTYPE.names}
    assert off == dict(tick=0, running=1, slots=2, fresh=3, matrix=4, swim=29, sums=45, nodes=52, node_max=53, node_id=54,
                       subjects=55, subject_id=56, subject_max=57, dead_time=58, reserved=63)
    src = open(HEADER).read()
    for k, name in enumerate(COLS):
        assert re.search(rf"#define SIM_GAZETTE_{name.upper()} {k}u", src), name


def test_the_observers_table_has_a_twelfth_entry():
    """The pinned line of the eight stays; the board, the catalogue and the gazette follow it."""
    src = open(os.path.join(ROOT, "serf_amd", "csrc", "serf_sim_host.inc")).read()
    assert "OB_TREE = 7, OB_N = 8 };" in src
    assert re.search(r"OB_CATALOG = OB_N \+ 1, OB_GAZETTE = OB_N \+ 2, OB_ALL = OB_N \+ 3", src)
    hip = open(os.path.join(ROOT, "serf_amd", "csrc", "serf_sim.hip")).read()
    assert hip.index('"serf_sim_catalog.inc"') < hip.index('"serf_sim_gazette.inc"')


def test_the_kernels_use_no_global_atomics_and_the_named_cap():
    """Every atomic in the file — called directly or through lds_sum / lds_max (serf_sim_observe.inc) — has `&name[` as its
    first argument, and every such name is declared __shared__ in the file."""
    src = re.sub(r"//.*", "", open(INC).read())
    shared = set(re.findall(r"__shared__\s+[\w\s\*]+?\b(\w+)\s*\[", src))
    calls = re.findall(r"\b(atomic\w+|lds_sum|lds_max)\s*\(\s*([^,]+),", src)
    assert len(calls) >= 10
    for fn, first in calls:
        m = re.fullmatch(r"&(\w+)\[.*", first.strip())
        assert m and m.group(1) in shared, f"{fn}({first}, ...): not an LDS array of this file"
    assert {"acc", "s_cnt", "hdr", "kmax"} <= shared
    assert gazette_grid() == 1024 and second_n() == 262209


# ---- 2. the model's invariants ----
def check_invariants(r, window=WINDOW):
    s, nodes, subj = r["samples"], r["nodes"].astype(np.int64), r["subjects"].astype(np.int64)
    assert len(s) == r["count"][0] and (s["reserved"] == 0).all()
    sums = s["sums"].astype(np.int64)
    assert nodes[:, :7].sum(axis=0).tolist() == subj[:, :7].sum(axis=0).tolist() == sums.sum(axis=0).tolist()
    mat, swim = s["matrix"].astype(np.int64), s["swim"].astype(np.int64)
    assert (mat[:, range(5), range(5)] == 0).all() and (swim[:, range(4), range(4)] == 0).all()
    A, L, F = _ffi.STATUS_ALIVE, _ffi.STATUS_LEFT, _ffi.STATUS_FAILED
    assert (sums[:, 0] == mat[:, 0, 1:].sum(axis=1) + mat[:, L, A] + mat[:, F, A]).all()                 # join
    assert (sums[:, 1] == mat[:, 1:, L].sum(axis=1)).all() and (sums[:, 2] == mat[:, 1:, F].sum(axis=1)).all()
    assert (sums[:, 3] == mat[:, 1:, 0].sum(axis=1)).all()                                               # reap
    assert (sums[:, 5] == swim[:, 0, 1]).all() and (sums[:, 6] == swim[:, 1, 0]).all()
    assert (sums[:, 4] <= sums[:, 0]).all() and (s["dead_time"].astype(np.int64).sum(axis=1) == mat[:, F, A]).all()
    assert (sums[:, 4] <= mat[:, F, A]).all()
    assert (s["fresh"] <= s["slots"]).all() and (s["nodes"] <= s["running"]).all() and (s["subjects"] <= s["slots"]).all()
    assert ((s["node_max"] > 0) == (s["nodes"] > 0)).all() and ((s["subject_max"] > 0) == (sums[:, 2] > 0)).all()
    if len(s):
        assert nodes[:, 7].max() == s["node_max"].max() and subj[:, 7].max() == s["subject_max"].max()


@pytest.mark.parametrize("name,arg", [("main", ("krandomnodes", 1)), ("main", ("bijection", 3)), ("recycle", 1), ("recycle", 5),
                                      ("ragged", 65), ("idle", None), ("groups", None)])
def test_invariants_of_the_model_at_every_sample(name, arg):
    check_invariants(run(name, arg))


def test_main_is_nontrivial_on_the_oracle():
    for fan in ("krandomnodes", "bijection"):
        r = run("main", (fan, 1))
        tl.inside_bounds(r["o"])
        tot = r["samples"]["sums"].astype(np.int64).sum(axis=0)
        assert (tot[:4] > 0).all() and tot[5] > 0, tot                                  # all four events, suspicions
        assert 0 < tot[4] < r["samples"]["matrix"].astype(np.int64)[:, 4, 1].sum(), "flaps inside the window and joins outside it"
        assert tot[2] >= 5 * (N - 6), "six crashed members, each announced by nearly every running node"
        assert r["samples"]["fresh"].sum() == 8, "the six crashed nodes and the two leavers get their slots while the gazette runs"
        assert r["samples"]["running"].min() < N and (r["nodes"][script(N)["crashed"][2], :4] == 0).all(), "a stopped node sees nothing"
    p3 = run("main", ("krandomnodes", 3))
    assert len(p3["samples"]) == -(-TICKS // 3) and p3["samples"]["tick"].tolist() == list(range(1, TICKS + 1, 3))


def edge_window():
    """A dead time that main's joins out of Failed really have, and not the smallest: as flap_window it is the boundary."""
    ages = sorted(set(run("main", ("krandomnodes", 1))["m"].ages))
    return ages[len(ages) // 4]


def test_flap_window_is_exclusive():
    """flap_window = a dead time that occurs: those joins are no flaps, with one tick more they are."""
    w = edge_window()
    at = run("main", ("krandomnodes", 1, w))["samples"]["sums"].astype(np.int64)[:, 4].sum()
    above = run("main", ("krandomnodes", 1, w + 1))["samples"]["sums"].astype(np.int64)[:, 4].sum()
    hits = run("main", ("krandomnodes", 1))["m"].ages.count(w)
    assert hits > 0 and above - at == hits and at > 0


def test_recycle_rehomes_slots_between_two_samples():
    for period in (1, 5):
        r = run("recycle", period)
        cs = r["o"].cluster_stats()
        assert cs["slots_recycled"] >= 8
        assert r["m"].rehomed >= 2, "no slot ever went to another subject between two samples"
        tot = r["samples"]["sums"].astype(np.int64).sum(axis=0)
        assert tot[5] > 0 and tot[6] > 0, "suspicions raised and cleared (a node is down for four ticks: nobody is declared Failed)"


def test_boundary_ties_rows_255_and_256():
    r = run("boundary")
    check_invariants(r)
    f = r["subjects"][:, 2]
    assert f[255] == f[256] == 255 and not f[:255].any(), "every running node announced both Failed, and nobody else"


def test_idle_counts_nothing_while_the_shadow_moves():
    r = run("idle")
    s = r["samples"]
    after = s["running"] == 0
    assert after.any() and (s["sums"][after] == 0).all() and (s["matrix"][after] == 0).all() and (s["nodes"][after] == 0).all()


def test_sampling_rule_and_full_buffer_of_the_model(oracle):
    o = _ffi.Sim(oracle, _ffi.make_config(256, **dict(shapes.KW, view_slots=16)))
    m = GazetteModel(o)
    o.inject(6, _ffi.OP_CRASH, 9)
    m.step(4)
    m.start(first_tick=10, period=7, capacity=3)
    m.step(40)
    assert m.count() == (3, 2) and m.read()["tick"].tolist() == [11, 18, 25]                # 31, 38 dropped
    m.stop()
    m.start(first_tick=0, period=2, capacity=100)
    m.step(5)
    assert m.count() == (3, 0) and m.read()["tick"].tolist() == [45, 47, 49]


def test_gazette_rates():
    r = run("main", ("krandomnodes", 1))
    g = _ffi.gazette_rates(r["samples"], r["nodes"])
    tot = r["samples"]["sums"].astype(np.int64).sum(axis=0)
    assert g["ticks"] == TICKS and g["totals"] == {name: int(tot[k]) for k, name in enumerate(COLS[:7])}
    assert g["per_tick"]["flap"] == tot[4] / TICKS
    ev = np.sort(r["nodes"][:, :4].astype(np.int64).sum(axis=1))
    assert g["per_node"] == dict(median=int(ev[N // 2 - 1]), p99=int(ev[989]), max=int(ev[-1]))


# ---- 3. the model against the oracle's event log ----
EVENT_COLUMN = {_ffi.EV_JOIN: 0, _ffi.EV_LEAVE: 1, _ffi.EV_FAILED: 2, _ffi.EV_REAP: 3}


def test_model_counts_what_the_event_log_says():
    """main on the oracle with every node watched, period 1.  Per tick, every (observer, subject) pair with exactly one member
    event (Join / Leave / Failed / Reap; SIM_EV_UPDATE is out of the gazette's scope and not looked at) whose entry was not
    already Alive or Leaving before a SIM_EV_JOIN: the model counts exactly that event's column.  Every pair without an event
    counts nothing in columns 0-3.  Pairs outside the condition are excluded, and counted."""
    n, kw, drive, start = scenario("main", ("krandomnodes", 1))
    o = tl.maker(n, kw)()
    for x in range(n):
        o.watch(x)
    m = GazetteModel(o)
    m.start(**start)
    slots = {}                                                   # tick -> {subject: (columns 0-3 [4][n], s(prev) [n])}
    m.on_slot = lambda t, x, cols, sp: slots.setdefault(t, {}).__setitem__(x, (cols[:4].copy(), sp.copy()))
    log = {}

    def on_tick():
        t = o.tick - 1
        while True:
            evs = o.drain_events()
            for tick, obs, typ, key, ltime in evs:
                if typ in EVENT_COLUMN:
                    assert tick == t
                    log.setdefault(t, {}).setdefault((obs, key), []).append(typ)
            if len(evs) < 65536:
                break
    m.on_tick = on_tick
    drive(o, m.step)
    compared, excluded, types, silent, why = 0, 0, set(), 0, {}
    for t in range(TICKS):
        seen = slots.get(t, {})
        handled = set()
        for (obs, x), typs in log.get(t, {}).items():
            handled.add((obs, x))
            assert x in seen, f"tick {t}: an event about subject {x}, which has no slot"
            cols, sp = seen[x]
            if len(typs) != 1 or (typs[0] == _ffi.EV_JOIN and sp[obs] in (_ffi.STATUS_ALIVE, _ffi.STATUS_LEAVING)):
                excluded += 1
                why[(t // 10 * 10, x, tuple(typs), int(sp[obs]))] = why.get((t // 10 * 10, x, tuple(typs), int(sp[obs])), 0) + 1
                continue
            want = [int(k == EVENT_COLUMN[typs[0]]) for k in range(4)]
            assert cols[:, obs].astype(int).tolist() == want, f"tick {t}: observer {obs}, subject {x}: event {typs[0]}, model {cols[:, obs]}"
            compared += 1
            types.add(typs[0])
        for x, (cols, sp) in seen.items():                       # every pair without an event counts nothing
            for obs in np.nonzero(cols.any(axis=0))[0].tolist():
                assert (obs, x) in handled, f"tick {t}: observer {obs}, subject {x}: the model counts {cols[:, obs]}, the log has no event"
            silent += n - int(cols.any(axis=0).sum())
    with_events = compared + excluded
    assert excluded * 20 <= with_events, (excluded, with_events, why)
    assert compared >= 1000 and types == set(EVENT_COLUMN) and silent > 0, (compared, types)
    s = m.read()
    back = s["matrix"].astype(np.int64)[:, 4, 1].sum()
    flaps = s["sums"].astype(np.int64)[:, 4].sum()
    assert 0 < flaps < back, "one revive inside flap_window, one outside"
    # watching changes nothing the gazette sees
    plain = run("main", ("krandomnodes", 1))
    assert s.tobytes() == plain["samples"].tobytes() and (m.nodes == plain["nodes"]).all() and (m.subj == plain["subjects"]).all()


def test_classify_on_literal_words():
    """The columns on hand-made bits words: known | status << 1 | swim << 4 | stamp << 11."""
    def b(status, swim=0, stamp=0):
        return (1 | status << 1 | swim << 4 | stamp << 11) if status else 0
    A, G, L, F = _ffi.STATUS_ALIVE, _ffi.STATUS_LEAVING, _ffi.STATUS_LEFT, _ffi.STATUS_FAILED
    cases = [(0, b(A), "join"), (b(L), b(A), "join"), (b(F, 2, 40), b(A), "join flap"), (b(F, 2, 40), b(A, 0, 99), "join flap"),
             (b(F, 2, 39), b(A), "join"), (b(G), b(A), ""), (b(A), b(L, 3), "leave"), (b(G), b(L, 3), "leave"), (b(F), b(L), "leave"),
             (b(A), b(F, 2), "failed"), (b(L), b(F), "failed"), (b(A), 0, "reap"), (b(F), 0, "reap"), (0, b(F), "join"),
             (b(A), b(A, 1), "suspected"), (b(A, 1), b(A), "cleared"), (b(A, 1), b(A, 2), ""), (b(A), b(A, 0, 7), "")]
    for prev, cur, want in cases:
        cols, _ = classify(np.array([prev]), np.array([cur]), 100, 61)
        got = " ".join(name for k, name in enumerate(COLS[:7]) if cols[k][0])
        assert got == want, (hex(prev), hex(cur), got, want)
    cols, _ = classify(np.array([b(F, 2, 40)]), np.array([b(A)]), 100, 60)                  # age 60 is not < 60
    assert not cols[4][0]
    cols, _ = classify(np.array([b(F, 2, 0x1FFFFE)]), np.array([b(A)]), 3, 60)             # the stamp wraps: age 5
    assert cols[4][0]
