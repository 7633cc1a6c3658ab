"""The spread map of the HIP library (include/serf_sim_spread.h) against the reference model (tests/spread_model.py) on the
oracle stepped one tick at a time: the scenarios of tests/test_spread.py, the observer shapes of tests/test_observer_shapes.py
(ragged, idle, second pass: spread_latch_kernel and the summary's passes have the series' pass loop and grid cap), the sampling
rules, neutrality, the errors, and a map that exists before a restore.  The HIP handle advances in long sim_step calls and is
read once at the end; every operation is injected up front, the entries' Lamport times are the oracle's; every word of the
samples, of the map and of its three reads is compared exactly, and the digest equals the oracle's in every test."""
import functools

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_ledger as tl
from tests import test_observer_shapes as shapes
from tests import test_spread as tsp
from tests.spread_model import SpreadModel

pytestmark = pytest.mark.gpu
HW, EW = _ffi.SPREAD_HEADER_WORDS, _ffi.SPREAD_ENTRY_WORDS
ARRAYS = (_ffi.ARR_ROWS, _ffi.ARR_QUEUE, _ffi.ARR_INBOX, _ffi.ARR_VIEW, _ffi.ARR_ERING, _ffi.ARR_QRING, _ffi.ARR_SLOTMAP)


def words(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1)


def same_samples(got, want, what):
    """(headers, records) of the library against the model's, word for word."""
    (gh, gr), (wh, wr) = got, want
    assert gh.shape == wh.shape and gr.shape == wr.shape, f"{what}: {gh.shape} {gr.shape} != {wh.shape} {wr.shape}"
    for f in ("tick", "running", "n", "new", "started", "full"):
        bad = np.nonzero(gh[f] != wh[f])[0]
        assert not len(bad), f"{what}: header.{f} of sample {bad[0]}: HIP {gh[f][bad[0]]} != model {wh[f][bad[0]]}"
    for f in _ffi.SPREAD_ENTRY_DTYPE.names:
        bad = np.argwhere(gr[f] != wr[f])
        assert not len(bad), f"{what}: {f} of sample {bad[0][0]}, entry {bad[0][1]}: HIP {gr[f][tuple(bad[0])]} != model {wr[f][tuple(bad[0])]}"
    assert words(gh).tolist() == words(wh).tolist() and words(gr).tolist() == words(wr).tolist()


def same_records(got, want, what):
    for f in want.dtype.names:
        bad = np.argwhere(np.asarray(got[f] != want[f]))
        assert not len(bad), f"{what}: {f} at {bad[0].tolist()}: HIP {got[f][tuple(bad[0])]} != model {want[f][tuple(bad[0])]}"
    assert words(got).tolist() == words(want).tolist(), what


def same_reads(g, m, what, top_ks=(1, 7, 64)):
    """The whole map, every summary word at bin_width 1 and 3, the full unreached lists and a cap below the total, and
    spread_late for both orders with every node's record."""
    n = int(g.cfg.n_nodes)
    for e in range(len(m.entries)):
        got = g.spread_map(e)
        bad = np.nonzero(got != m.map(e))[0]
        assert not len(bad), f"{what}: arrival[{e}][{bad[0]}]: HIP {got[bad[0]]} != model {m.map(e)[bad[0]]}"
        ids, total = g.spread_unreached(e)
        wids, wtotal = m.unreached(e)
        assert total == wtotal and ids.tolist() == wids.tolist(), f"{what}: unreached of entry {e}"
        cap = max(0, wtotal - 3) if wtotal > 3 else wtotal // 2
        ids, total = g.spread_unreached(e, cap)
        assert total == wtotal and ids.tolist() == wids[:cap].tolist(), f"{what}: unreached of entry {e}, cap {cap}"
    if n > 5:
        assert g.spread_map(0, 2, 3).tolist() == m.map(0, 2, 3).tolist() and len(g.spread_map(0, n, 0)) == 0
    for bw in (1, 3):
        same_records(g.spread_summary(bw), m.summary(bw), f"{what}: summary, bin_width {bw}")
    for rank_by in (_ffi.SPREAD_BY_MISSED, _ffi.SPREAD_BY_LATE):
        for k in top_ks:
            top, every = g.spread_late(k, rank_by, nodes=True)
            wtop, wevery = m.late(k, rank_by, nodes=True)
            same_records(every, wevery, f"{what}: every node's record")
            same_records(top, wtop, f"{what}: top {k} by {rank_by}")
            same_records(g.spread_late(k, rank_by), wtop, f"{what}: top {k} by {rank_by} without nodes")


def same_run(n, kw, script, run, what, **start):
    """The scenario on the HIP library, read once at the end, against the cached oracle run."""
    o, m, entries, want = run["o"], run["m"], run["entries"], run["samples"]
    g = serf_amd.create(n, **kw)
    g.spread_start(entries, **start)
    script(g, g.step)
    assert g.spread_count() == (len(want[0]), m.count()[1])
    same_samples(g.spread_read(), want, what)
    same_reads(g, m, what)
    assert g.digest() == o.digest(), what
    return g


# ---- 1. the baseline scenarios ----
@pytest.mark.parametrize("variant", tsp.VARIANTS)
@pytest.mark.parametrize("name", ("lives", "dies"))
def test_lives_and_dies_512_nodes_every_tick(hiplib, name, variant):
    run = tsp.oracle_run(name, variant)
    if variant == "krandomnodes":
        (tsp.check_lives if name == "lives" else tsp.check_dies)(run)
    assert run["samples"][1]["reached"][-1].max() > tsp.N // 2
    same_run(tsp.N, tsp.variant_kw(name, variant), tsp.drive, run, f"{name} {variant}", capacity=tsp.TICKS).close()


# ---- 2. the series scenario ----
def test_series_scenario_64_entries_of_four_kinds_and_an_overflow_row(hiplib):
    run = tsp.series_oracle()
    tsp.check_series(run)
    same_run(tsp.SERIES_N, tsp.SERIES_KW, tsp.series_drive, run, "series", capacity=tsp.SERIES_TICKS).close()


# ---- 3. shapes ----
def none(spec):
    return None


def ragged_drive(n):
    return lambda sim, step: shapes.ragged_script(sim, n, none, step)


RAGGED_SIZES = (1, 2, 63, 64, 65, 257, 1025)


@functools.lru_cache(maxsize=None)
def ragged_oracle(n, fan):
    make = tl.maker(n, shapes.ragged_kw(n, fan))
    dry = make()
    _, ru = shapes.ragged_script(dry, n, none, dry.step)       # the rumours' Lamport times
    dry.close()
    entries = list(dict.fromkeys(shapes.five_rumours(ru, n)))
    o, m, seen, _ = tsp.model_run(make, ragged_drive(n), entries, capacity=shapes.RAGGED_TICKS)
    return dict(o=o, m=m, entries=entries, samples=m.read(), seen=seen)


@pytest.mark.parametrize("fan", sorted(shapes.FANOUTS))
@pytest.mark.parametrize("n", RAGGED_SIZES)
def test_ragged_sizes(hiplib, n, fan):
    run = ragged_oracle(n, fan)
    hdr, rec = run["samples"]
    tl.inside_bounds(run["o"])
    assert rec["holds"].tolist() == run["seen"]
    assert hdr["running"][0] == n and hdr["running"][-1] == max(1, n - 2) and rec["reached"][-1].max() == n
    assert {e[0] for e in run["entries"]} == {_ffi.K_JOIN, _ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY}
    if n > 2:
        assert (rec["reached"][-1] > rec["reached_up"][-1]).any(), "the crashed node had an arrival"
    same_run(n, shapes.ragged_kw(n, fan), ragged_drive(n), run, f"ragged({n}) {fan}", capacity=shapes.RAGGED_TICKS).close()


IDLE_ENTRIES = [(_ffi.K_EVENT, shapes.EVENT_KEY, 99), (_ffi.K_JOIN, 0, 1), (_ffi.K_LEAVE, 0, 2)]


def idle_drive(n):
    return lambda sim, step: shapes.idle_script(sim, n, none, step)


@pytest.mark.parametrize("n", shapes.IDLE_SIZES)
def test_nobody_runs(hiplib, n):
    """Behind the crash of every node: every count of the running is 0, every list empty; the arrivals latched before stay."""
    kw = dict(shapes.KW, view_slots=0, flags=shapes.FANOUTS["krandomnodes"])
    o, m, seen, _ = tsp.model_run(tl.maker(n, kw), idle_drive(n), IDLE_ENTRIES, capacity=shapes.IDLE_TICKS)
    hdr, rec = m.read()
    assert hdr["running"].tolist() == [n] * shapes.IDLE_CRASH + [0] * (shapes.IDLE_TICKS - shapes.IDLE_CRASH)
    late = slice(shapes.IDLE_CRASH, None)
    assert not hdr["new"][late].any() and not hdr["full"][late].any() and not rec["holds"][late].any() and not rec["reached_up"][late].any()
    assert rec["reached"][-1].tolist() == [0, n, 0] and rec["first"][-1].tolist() == [0, 1, 0]
    assert all(m.unreached(e)[1] == 0 for e in range(3)) and not words(m.late(64)).any() and not m.summary(1)["unreached_up"].any()
    run = dict(o=o, m=m, entries=IDLE_ENTRIES, samples=(hdr, rec))
    same_run(n, kw, idle_drive(n), run, f"nobody_runs({n})", capacity=shapes.IDLE_TICKS).close()


def big_drive(sim, step):
    shapes.big_start(sim, shapes.SERIES_N)
    step(shapes.SERIES_TICKS)


@functools.lru_cache(maxsize=None)
def second_pass_oracle():
    n = shapes.SERIES_N
    make = tl.maker(n, shapes.BIG_KW)
    o = make()
    ev = shapes.big_start(o, n)
    o.close()
    entries = [ev, (_ffi.K_JOIN, n - 1, 1)]
    o, m, seen, _ = tsp.model_run(make, big_drive, entries, period=shapes.SERIES_PERIOD, capacity=100)
    return dict(o=o, m=m, entries=entries, samples=m.read(), seen=seen)


def test_second_pass(hiplib):
    """SPREAD_GRID * BLOCK + 65 nodes: the pass loops of spread_latch_kernel, spread_stat_kernel and spread_hist_kernel take a
    second turn, of one whole wave and one lane; the event's origin and the crashed node lie in that pass."""
    tsp.test_the_cap_is_the_sources()
    assert tsp.SPREAD_GRID * shapes.BLOCK + shapes.SECOND_PASS == shapes.SERIES_N == 262209
    run = second_pass_oracle()
    hdr, rec = run["samples"]
    n = shapes.SERIES_N
    assert hdr["tick"].tolist() == [1, 5, 9] and hdr["running"].tolist() == [n, n - 1, n - 1]
    assert rec["reached"][0].tolist() == [1, n] and rec["reached"][-1, 0] > 100 and rec["reached_up"][-1, 1] == n - 1
    assert run["m"].map(0)[n - 3] == 1 and run["m"].map(1)[n - 1] == 1, "the origin and the crashed node: nodes of the second pass"
    g = same_run(n, shapes.BIG_KW, big_drive, run, "second pass", period=shapes.SERIES_PERIOD, capacity=100)
    g.close()


# ---- 4. sampling ----
def pair(name="dies"):
    """A fresh oracle with its model and a fresh HIP handle, the scenario's events injected into both."""
    kw = tsp.variant_kw(name, "krandomnodes")
    o = tl.maker(tsp.N, kw)()
    g = serf_amd.create(tsp.N, **kw)
    for s in (o, g):
        for t, node, key in tsp.events():
            s.inject(t, _ffi.OP_USER_EVENT, node, key, 64)
    return o, SpreadModel(o), g


def test_period_first_tick_capacity_and_restart(hiplib):
    """Period 4 from a first tick in the future, a buffer three short of what the run would fill (a dropped sample latches
    nothing); a refused second start; a second map after sim_spread_stop begins empty, with other entries; partial reads."""
    entries = tsp.oracle_run("dies")["entries"]
    first, period, ticks = 5, 4, 40
    due = len(range(first, ticks, period))
    o, m, g = pair()
    m.start(entries, first, period, due - 3)
    g.spread_start(entries, first, period, due - 3)
    m.step(ticks)
    g.step(ticks)
    assert g.spread_count() == m.count() == (due - 3, 3)
    with pytest.raises(_ffi.SimError) as ei:
        g.spread_start(entries[:2], 0, 1, 8)          # one map at a time
    assert ei.value.code == _ffi.ESTATE and g.spread_count() == (due - 3, 3)
    want = m.read()
    assert want[0]["tick"].tolist() == [first + 1 + period * i for i in range(due - 3)] and want[1]["new"][0].sum() > 1
    same_samples(g.spread_read(), want, "period 4")
    same_samples(g.spread_read(2, 3), m.read(2, 3), "a partial read")
    same_samples(g.spread_read(due - 4), m.read(due - 4), "the last sample")
    assert g.spread_read(1, 0)[0].shape == (0,)
    same_reads(g, m, "period 4", top_ks=(7,))
    assert set(np.unique(g.spread_map(0)).tolist()) <= {0} | set(want[0]["tick"].tolist())
    g.spread_stop()
    m.stop()
    with pytest.raises(_ffi.SimError) as ei:
        g.spread_read(0, 0)
    assert ei.value.code == _ffi.ESTATE and g.spread_count() == (0, 0)
    other = [entries[4], (_ffi.K_JOIN, 3, 1), entries[1]]
    m.start(other, 0, 2, 5)                            # a first tick that has passed: now
    g.spread_start(other, 0, 2, 5)
    m.step(7)
    g.step(7)
    assert g.spread_count() == m.count() == (4, 0)
    got = g.spread_read()
    same_samples(got, m.read(), "restarted")
    assert got[0]["tick"].tolist() == [41, 43, 45, 47] and got[0]["n"].tolist() == [3] * 4
    assert got[1]["first"][0].tolist() == [41 if x else 0 for x in got[1]["reached"][0].tolist()], "a new map starts empty"
    same_reads(g, m, "restarted", top_ks=(7,))
    assert g.digest() == o.digest()
    g.close()


def test_one_step_call_against_single_steps_and_reads_in_between(hiplib):
    """sim_step(h, 40) against forty sim_step(h, 1) with a read of the map, a summary, an unreached list and a ranking between
    them: the same samples and the same map — a read changes nothing."""
    run = tsp.oracle_run("dies")
    entries, ticks = run["entries"], 40
    _, _, a = pair()
    _, _, b = pair()
    a.spread_start(entries, 0, 1, ticks)
    b.spread_start(entries, 0, 1, ticks)
    a.step(ticks)
    for t in range(ticks):
        b.step(1)
        if t % 7 == 3:
            b.spread_map(t % len(entries))
            b.spread_summary(2)
            b.spread_unreached(0, 5)
            b.spread_late(3, _ffi.SPREAD_BY_LATE, nodes=True)
    same_samples(a.spread_read(), b.spread_read(), "step(40) against 40 step(1) with reads between them")
    want = run["samples"]
    same_samples(b.spread_read(), (want[0][:ticks], want[1][:ticks]), "the model's first 40 samples")
    for e in range(len(entries)):
        assert a.spread_map(e).tolist() == b.spread_map(e).tolist()
    assert a.digest() == b.digest()
    a.close()
    b.close()


# ---- 5. neutrality ----
def test_a_running_map_changes_no_protocol_state(hiplib):
    """The series scenario with a map and without: equal digests, equal dumps of all seven arrays, equal images.  A handle that
    never started a map reports none and has nothing to read (its entry of the observers' table is null: sim_step_end passes it
    by — the library has no launch counter to show that with)."""
    run = tsp.series_oracle()
    with_map = serf_amd.create(tsp.SERIES_N, **tsp.SERIES_KW)
    without = serf_amd.create(tsp.SERIES_N, **tsp.SERIES_KW)
    with_map.spread_start(run["entries"], 0, 1, tsp.SERIES_TICKS)
    tsp.series_drive(with_map, with_map.step)
    tsp.series_drive(without, without.step)
    assert with_map.spread_count() == (tsp.SERIES_TICKS, 0) and without.spread_count() == (0, 0)
    assert with_map.digest() == without.digest() == run["o"].digest()
    for which in ARRAYS:
        assert with_map.dump(which).tobytes() == without.dump(which).tobytes(), f"dump {which}"
    assert with_map.snapshot().tobytes() == without.snapshot().tobytes(), "an image holds no map"
    assert with_map.cluster_stats() == without.cluster_stats()
    for call in (lambda: without.spread_read(0, 0), without.spread_stop, lambda: without.spread_map(0), without.spread_summary,
                 lambda: without.spread_unreached(0), without.spread_late):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    with_map.close()
    without.close()


# ---- 6. errors and states ----
def test_errors_leave_everything_as_it_was(hiplib):
    n = tsp.N
    kw = tsp.variant_kw("lives", "krandomnodes")
    ok = [(_ffi.K_EVENT, 0x77, 3), (_ffi.K_LEAVE, 5, 2), (_ffi.K_JOIN, 9, 1)]
    sh = serf_amd.create(n, force_sharded=True, **kw)      # a shard has no map
    every = lambda s: (lambda: s.spread_start(ok), s.spread_count, lambda: s.spread_read(0, 0), s.spread_stop, lambda: s.spread_map(0, 0, 1),
                       s.spread_summary, lambda: s.spread_unreached(0), s.spread_late)
    for call in every(sh):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    g = serf_amd.create(n, **kw)
    assert g.spread_count() == (0, 0)
    for call in every(g)[2:]:                                              # no map yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    bad = [[], [(_ffi.K_JOIN, i, 1) for i in range(65)], [(0, 1, 1)], [(_ffi.K_ALIVE, 1, 0)], [(_ffi.K_SUSPECT, 1, 0)], [(_ffi.K_DEAD, 1, 0)],
           [(8, 1, 1)], [(_ffi.K_JOIN, n, 1)], [(_ffi.K_LEAVE, n + 5, 1)], [(_ffi.K_EVENT, 0, 1)], [(_ffi.K_QUERY, 0, 1)],
           [(_ffi.K_EVENT, 5, 1 << 48)], [(_ffi.K_LEAVE, 5, 1 << 48)], ok + [ok[1]], [ok[0], ok[0]]]
    for es in bad:
        with pytest.raises(_ffi.SimError) as ei:
            g.spread_start(es, 0, 1, 8)
        assert ei.value.code == _ffi.EINVAL and g.spread_count() == (0, 0), es
    for args in ((0, 0, 8), (0, 1, 0), (0, 1, _ffi.SPREAD_MAX_SAMPLES + 1)):
        with pytest.raises(_ffi.SimError) as ei:
            g.spread_start(ok, *args)
        assert ei.value.code == _ffi.EINVAL and g.spread_count() == (0, 0)
    f = g.lib.f
    assert f["spread_start"](g.h, None, 3, 0, 1, 8) == _ffi.EINVAL and f["spread_start"](None, _ffi.spread_entries(ok), 3, 0, 1, 8) == _ffi.EINVAL
    # arguments that can be judged without a map are SIM_EINVAL before "no map" is SIM_ESTATE
    buf = np.zeros(4096, np.uint64)
    u = _ffi.C.c_uint32
    a, b = u(77), u(78)
    ref = _ffi.C.byref
    assert f["spread_summary"](g.h, 0, buf.ctypes.data) == _ffi.EINVAL and f["spread_summary"](g.h, 1, None) == _ffi.EINVAL
    assert f["spread_map"](g.h, 0, 0, 1, None) == _ffi.EINVAL
    assert f["spread_unreached"](g.h, 0, None, 4, ref(a), ref(b)) == _ffi.EINVAL
    assert f["spread_unreached"](g.h, 0, buf.ctypes.data, 4, None, ref(b)) == _ffi.EINVAL
    assert f["spread_unreached"](g.h, 0, buf.ctypes.data, 4, ref(a), None) == _ffi.EINVAL
    for top_k, rank_by in ((0, 0), (65, 0), (8, 2)):
        assert f["spread_late"](g.h, top_k, rank_by, buf.ctypes.data, None) == _ffi.EINVAL
    assert f["spread_late"](g.h, 8, 0, None, None) == _ffi.EINVAL
    assert (a.value, b.value) == (77, 78) and not buf.any()
    g.inject(1, _ffi.OP_CRASH, 9)
    lt = g.stats(3).event_time                                             # the Lamport time the event is about to get
    g.user_event(3, 0x77, 64)
    g.spread_start([(_ffi.K_EVENT, 0x77, lt)] + ok[1:], 0, 1, 8)
    g.step(3)
    assert g.spread_count() == (3, 0)
    before = g.spread_read()
    maps = [g.spread_map(e).tolist() for e in range(3)]
    assert before[0]["tick"].tolist() == [1, 2, 3] and before[1].shape == (3, 3) and before[1]["reached"][-1, 0] > 1
    for es in bad[:4]:                                                     # bad arguments before "already running"
        with pytest.raises(_ffi.SimError) as ei:
            g.spread_start(es, 0, 1, 8)
        assert ei.value.code == _ffi.EINVAL
    with pytest.raises(_ffi.SimError) as ei:
        g.spread_start(ok, 0, 0, 8)
    assert ei.value.code == _ffi.EINVAL
    with pytest.raises(_ffi.SimError) as ei:
        g.spread_start(ok, 0, 1, 8)
    assert ei.value.code == _ffi.ESTATE
    for first, cnt in ((0, 4), (3, 1), (4, 0)):                           # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.spread_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL and g.spread_count() == (3, 0)
    stride = HW + EW * 3
    got = u(77)
    small = np.zeros(2 * stride, np.uint64)
    assert f["spread_read"](g.h, 0, 3, small.ctypes.data, small.size, ref(got)) == _ffi.EINVAL         # a buffer one sample short
    assert f["spread_read"](g.h, 0, 2, None, small.size, ref(got)) == _ffi.EINVAL and f["spread_read"](g.h, 0, 2, small.ctypes.data, small.size, None) == _ffi.EINVAL
    assert got.value == 77 and not small.any()
    assert f["spread_count"](g.h, None, ref(b)) == _ffi.EINVAL and f["spread_count"](g.h, ref(a), None) == _ffi.EINVAL
    assert f["spread_count"](None, ref(a), ref(b)) == _ffi.EINVAL
    # an entry or nodes out of the running map's range
    out32 = np.zeros(n + 1, np.uint32)
    for entry, first, cnt in ((3, 0, 1), (0, n, 1), (0, 0, n + 1), (0, n - 1, 2), (0, 0xFFFFFFFF, 2)):
        assert f["spread_map"](g.h, entry, first, cnt, out32.ctypes.data) == _ffi.EINVAL
    assert f["spread_unreached"](g.h, 3, out32.ctypes.data, 4, ref(a), ref(b)) == _ffi.EINVAL
    assert f["spread_summary"](g.h, 0, buf.ctypes.data) == _ffi.EINVAL
    assert f["spread_late"](g.h, 65, 0, buf.ctypes.data, None) == _ffi.EINVAL and f["spread_late"](g.h, 8, 2, buf.ctypes.data, None) == _ffi.EINVAL
    assert (a.value, b.value) == (77, 78) and not buf.any() and not out32.any()
    ids, total = g.spread_unreached(0, 0)                                  # cap 0: the count alone, no list
    assert len(ids) == 0 and total == g.spread_summary(1)["unreached_up"][0] > 0
    after = g.spread_read()
    assert g.spread_count() == (3, 0) and words(after[0]).tolist() == words(before[0]).tolist() and words(after[1]).tolist() == words(before[1]).tolist()
    assert [g.spread_map(e).tolist() for e in range(3)] == maps
    g.close()
    t = serf_amd.create(256, fanout=3)                                   # inside a tick
    t.spread_start(ok, 0, 1, 8)
    t.step(2)
    t.step_begin()
    for call in every(t):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                                   # a handle destroyed with a map running
    g.spread_start(ok, 0, 1, 4)
    g.step(6)
    assert g.spread_count() == (4, 2) and g.spread_read()[0]["tick"].tolist() == [1, 2, 3, 4]
    g.close()


# ---- 7. restore ----
RESTORE_T = 8


def test_a_map_that_exists_before_a_restore(hiplib):
    """sim_restore takes a handle at tick 0 only, so a map cannot hold arrivals when its handle is restored; what is reachable:
    a map started at tick 0 on a fresh handle that is then restored to tick 8 of `dies` — two events travelling, four still to
    be sent.  The restore leaves the map as it is: its samples go on behind the ticks t >= 8, nothing is counted as dropped, and
    a node that had a rumour in the image is latched at the first sample.  The reference: the model on an oracle that restores
    the same image.  A snapshot of the handle while the map runs is the image of a handle without one."""
    kw = tsp.variant_kw("dies", "krandomnodes")
    entries = tsp.oracle_run("dies")["entries"]
    src = tl.maker(tsp.N, kw)()
    tsp.drive(src, src.step, RESTORE_T)
    img = src.snapshot()
    o = tl.maker(tsp.N, kw)()
    m = SpreadModel(o)
    g = serf_amd.create(tsp.N, **kw)
    m.start(entries, 0, 1, tsp.TICKS)
    g.spread_start(entries, 0, 1, tsp.TICKS)
    o.restore(img)
    g.restore(img)
    assert g.tick == o.tick == RESTORE_T and g.spread_count() == (0, 0)
    m.step(20)
    g.step(20)
    assert g.snapshot().tobytes() == o.snapshot().tobytes()
    m.step(tsp.TICKS - RESTORE_T - 20)
    g.step(tsp.TICKS - RESTORE_T - 20)
    assert g.spread_count() == m.count() == (tsp.TICKS - RESTORE_T, 0)
    want = m.read()
    assert want[0]["tick"][0] == RESTORE_T + 1 and want[1]["new"][0, :2].min() > 1 and not want[1]["new"][0, 3:].any()
    same_samples(g.spread_read(), want, "a map that exists before a restore")
    same_reads(g, m, "a map that exists before a restore", top_ks=(7,))
    ref = tsp.oracle_run("dies")                      # the run that never restored: the same cluster from tick 8 on
    assert want[1]["holds"].tolist() == ref["samples"][1]["holds"][RESTORE_T:].tolist()
    assert g.digest() == o.digest()
    src.close()
    g.close()
