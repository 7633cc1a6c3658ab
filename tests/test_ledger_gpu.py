"""The rumour ledger of the HIP library (include/serf_sim_ledger.h) against the reference model (tests/ledger_model.py) on the
oracle stepped one tick at a time: the scenarios of tests/test_ledger.py, the observer shapes of tests/test_observer_shapes.py
(ragged, idle, second pass: ledger_count_kernel has the series' pass loop and grid cap), the rules, ledger_now, all five observers
on one handle, and the errors.  The HIP handle advances in long sim_step calls and is read once at the end; every operation is
injected up front, the entries' Lamport times are the oracle's; every word is compared exactly and the digest equals the
oracle's in every test."""
import functools

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_ledger as tl
from tests import test_observer_shapes as shapes
from tests import test_track_gpu as tt
from tests._oracle import load_oracle
from tests.census_model import CensusModel
from tests.ledger_model import LedgerModel
from tests.roll_model import RollModel
from tests.series_model import SeriesModel
from tests.test_census_gpu import assert_same as census_same
from tests.test_roll_gpu import assert_same as roll_same
from tests.test_series_gpu import assert_same as series_same
from tests.track_model import TrackModel

pytestmark = pytest.mark.gpu
HW, EW = _ffi.LEDGER_HEADER_WORDS, _ffi.LEDGER_ENTRY_WORDS


def words(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1)


def assert_same(got, want, what):
    """(headers, records) of the library against the model's, word for word."""
    (gh, gr), (wh, wr) = got, want
    assert gh.shape == wh.shape and gr.shape == wr.shape, f"{what}: {gh.shape} {gr.shape} != {wh.shape} {wr.shape}"
    for f in _ffi.LEDGER_HEADER_DTYPE.names:
        bad = np.nonzero(gh[f] != wh[f])[0]
        assert not len(bad), f"{what}: header.{f} of sample {bad[0]}: HIP {gh[f][bad[0]]} != model {wh[f][bad[0]]}"
    for f in _ffi.LEDGER_ENTRY_DTYPE.names:
        bad = np.argwhere(gr[f] != wr[f])
        assert not len(bad), f"{what}: {f} of sample {bad[0][0]}, entry {bad[0][1]}: HIP {gr[f][tuple(bad[0])]} != model {wr[f][tuple(bad[0])]}"
    assert words(gh).tolist() == words(wh).tolist() and words(gr).tolist() == words(wr).tolist()


def hip_run(n, kw, drive, entries, first=0, period=1, capacity=1 << 12):
    g = serf_amd.create(n, **kw)
    g.ledger_start(entries, first, period, capacity)
    drive(g, g.step)
    return g


def same_run(n, kw, drive, run, what, **start):
    """The scenario on the HIP library, read once at the end, against the cached oracle run (oracle, entries, (headers, records))."""
    o, entries, want = run[:3]
    g = hip_run(n, kw, drive, entries, **start)
    assert g.ledger_count() == (len(want[0]), 0)
    got = g.ledger_read()
    assert_same(got, want, what)
    assert g.digest() == o.digest(), what
    g.close()
    return got


# ---- 1. a rumour that dies ----
def test_a_rumour_that_dies(hiplib):
    run = tl.dies_oracle(True)
    tl.check_dies(run)
    same_run(tl.N, tl.DIES_KW, tl.dies_drive, run, "dies", capacity=tl.DIES_TICKS)


def test_the_same_script_without_loss(hiplib):
    run = tl.dies_oracle(False)
    tl.check_lives(run)
    hdr, rec = same_run(tl.N, tl.LIVES_KW, tl.dies_drive, run, "lives", capacity=tl.DIES_TICKS)
    assert (rec["in_flight"].astype(np.int64).sum(axis=0) == 16 * tl.N).all() and (rec["reach"][-1] == hdr["running"][-1]).all()


# ---- 2. the fan-out models ----
@pytest.mark.parametrize("variant", tl.VARIANTS)
def test_census_scenarios_4096_nodes_every_tick(hiplib, variant):
    run = tl.census_oracle(variant)
    tl.check_census(variant, run)
    same_run(tl.N, tl.census_kw(variant), tl.census_ledger_drive, run, variant, capacity=tl.CENSUS_TICKS)


# ---- 3. deep queues, two pages, all seven kinds ----
def test_deep_queues_two_pages_all_seven_kinds(hiplib):
    run = tl.deep_oracle()
    tl.check_deep(run)
    same_run(tl.DEEP_N, tl.DEEP_KW, tl.deep_drive, run, "deep", capacity=tl.DEEP_TICKS)


# ---- 4. four pages ----
def test_four_pages(hiplib):
    run = tl.pages_oracle()
    tl.check_pages(run)
    same_run(tl.N, tl.PAGES_KW, tl.pages_drive, run, "pages", capacity=tl.PAGES_TICKS)


# ---- 5. one pair, several values ----
def test_one_pair_two_values(hiplib):
    run = tl.twice_oracle()
    assert tl.check_twice(run) == 2
    same_run(tl.TWICE_N, tl.TWICE_KW, tl.twice_drive, run, "twice", capacity=tl.TWICE_TICKS)


# ---- 6. a crowded index ----
def test_a_crowded_index(hiplib):
    tl.test_the_index_is_the_sources()
    run = tl.crowded_oracle()
    tl.check_crowded(run)
    same_run(tl.N, tl.DIES_KW, lambda sim, step: tl.dies_drive(sim, step, 30), run, "crowded", period=3, capacity=10)


# ---- 7. shapes ----
def none(spec):
    return None


def ragged_drive(n):
    return lambda sim, step: shapes.ragged_script(sim, n, none, step)


@functools.lru_cache(maxsize=None)
def ragged_oracle(n, fan):
    make = tl.maker(n, shapes.ragged_kw(n, fan))
    found, _ = tl.dry_run(make, ragged_drive(n), wire=True)
    # (a node alone queues nothing: three identities that are named whatever the size stand at the end of every list)
    fixed = [(_ffi.K_EVENT, shapes.EVENT_KEY, 1), (_ffi.K_JOIN, n - 1, 1), (_ffi.K_ALIVE, 0, 0)]
    entries = tl.deal(found, _ffi.LEDGER_MAX - len(fixed))
    entries += [e for e in fixed if e not in entries]
    o, m, _ = tl.model_run(make, ragged_drive(n), entries, capacity=shapes.RAGGED_TICKS)
    return o, entries, m.read()


@pytest.mark.parametrize("fan", sorted(shapes.FANOUTS))
@pytest.mark.parametrize("n", shapes.RAGGED_SIZES + (8,))
def test_ragged_sizes(hiplib, n, fan):
    run = ragged_oracle(n, fan)
    o, entries, (hdr, rec) = run
    tl.inside_bounds(o)
    assert hdr["running"][0] == n and hdr["running"][-1] == max(1, n - 2) and (n < 10 or rec["queued"].max() > 0)
    assert rec["reach"].max() == n and (n == 1 or rec["in_flight"].max() > 0)
    if n >= 3:
        assert {e[0] for e in entries} >= {_ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY, _ffi.K_SUSPECT} and rec["in_flight"].max() > 0
    same_run(n, shapes.ragged_kw(n, fan), ragged_drive(n), run, f"ragged({n}) {fan}", capacity=shapes.RAGGED_TICKS)


IDLE_ENTRIES = [(_ffi.K_EVENT, shapes.EVENT_KEY, 99), (_ffi.K_JOIN, 0, 1), (_ffi.K_ALIVE, 0, 0)]


def idle_drive(n):
    return lambda sim, step: shapes.idle_script(sim, n, none, step)


@pytest.mark.parametrize("fan", sorted(shapes.FANOUTS))
@pytest.mark.parametrize("n", shapes.IDLE_SIZES)
def test_nobody_runs(hiplib, n, fan):
    kw = dict(shapes.KW, view_slots=0, flags=shapes.FANOUTS[fan])
    o, m, _ = tl.model_run(tl.maker(n, kw), idle_drive(n), IDLE_ENTRIES, capacity=shapes.IDLE_TICKS)
    hdr, rec = m.read()
    assert hdr["running"].tolist() == [n] * shapes.IDLE_CRASH + [0] * (shapes.IDLE_TICKS - shapes.IDLE_CRASH)
    assert not hdr["queued"][shapes.IDLE_CRASH:].any() and not rec["reach"][shapes.IDLE_CRASH:].any()
    same_run(n, kw, idle_drive(n), (o, IDLE_ENTRIES, (hdr, rec)), f"nobody_runs({n}) {fan}", capacity=shapes.IDLE_TICKS)


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
    entries = [ev, (_ffi.K_JOIN, n - 1, 1), (_ffi.K_SUSPECT, n - 1, 0)]
    o, m, _ = tl.model_run(make, big_drive, entries, period=shapes.SERIES_PERIOD, capacity=100)
    return o, entries, m.read()


def test_second_pass(hiplib):
    """SER_CAP + 65 nodes: ledger_count_kernel's pass loop takes a second turn, of one whole wave and one lane; the event's origin
    and the crashed node lie in that pass."""
    assert shapes.SER_CAP == 1024 * 256 and tl.ledger_tab()       # (LEDGER_GRID 1024u: tl.test_the_index_is_the_sources)
    run = second_pass_oracle()
    o, entries, (hdr, rec) = run
    assert hdr["tick"].tolist() == [1, 5, 9] and hdr["running"].tolist() == [shapes.SERIES_N, shapes.SERIES_N - 1, shapes.SERIES_N - 1]
    assert rec["in_flight"][0, 0] == 4 and rec["holders"][0, 0] == 1 and rec["reach"][-1, 0] > rec["reach"][0, 0] == 1
    assert rec["queued"][-1, 2] > 0, "nobody suspects the crashed node yet"
    same_run(shapes.SERIES_N, shapes.BIG_KW, big_drive, run, "second pass", period=shapes.SERIES_PERIOD, capacity=100)


@pytest.mark.parametrize("count", (1, 64))
def test_one_entry_and_sixty_four(hiplib, count):
    o, entries, _, _, _, found = tl.deep_oracle()
    entries = entries[20:21] if count == 1 else entries
    o, m, _ = tl.model_run(tl.maker(tl.DEEP_N, tl.DEEP_KW), tl.deep_drive, entries, first=10, period=5, capacity=100)
    want = m.read()
    assert want[1].shape[1] == count and want[1]["queued"].max() > 0
    same_run(tl.DEEP_N, tl.DEEP_KW, tl.deep_drive, (o, entries, want), f"{count} entries", first=10, period=5, capacity=100)


# ---- 8. rules ----
def test_period_first_tick_capacity_and_restart(hiplib):
    """Period 7 from a first tick in the future, a buffer three short of what the run would fill; a refused second start; a
    second ledger after sim_ledger_stop begins at sample 0, with other entries; partial reads."""
    _, entries, _ = tl.dies_oracle(True)
    first, period, ticks = 5, 7, 60
    due = len(range(first, ticks, period))
    o = tl.maker(tl.N, tl.DIES_KW)()
    m = LedgerModel(o)
    g = serf_amd.create(tl.N, **tl.DIES_KW)
    for s in (o, g):
        for t, node, key in tl.dies_events():
            s.inject(t, _ffi.OP_USER_EVENT, node, key, 64)
    m.start(entries, first, period, due - 3)
    g.ledger_start(entries, first, period, due - 3)
    m.step(ticks)
    g.step(ticks)
    assert g.ledger_count() == m.count() == (due - 3, 3)
    with pytest.raises(_ffi.SimError) as ei:
        g.ledger_start(entries[:2], 0, 1, 8)          # one ledger at a time
    assert ei.value.code == _ffi.ESTATE and g.ledger_count() == (due - 3, 3)
    assert_same(g.ledger_read(), m.read(), "period 7")
    assert_same(g.ledger_read(2, 3), m.read(2, 3), "a partial read")
    assert_same(g.ledger_read(due - 4), m.read(due - 4), "the last sample")
    assert g.ledger_read(1, 0)[0].shape == (0,)
    g.ledger_stop()
    m.stop()
    with pytest.raises(_ffi.SimError) as ei:
        g.ledger_read(0, 0)
    assert ei.value.code == _ffi.ESTATE and g.ledger_count() == (0, 0)
    other = [entries[4], (_ffi.K_JOIN, 3, 1), entries[1]]
    m.start(other, 0, 2, 5)                            # a first tick that has passed: now
    g.ledger_start(other, 0, 2, 5)
    m.step(7)
    g.step(7)
    assert g.ledger_count() == m.count() == (4, 0)
    got = g.ledger_read()
    assert_same(got, m.read(), "restarted")
    assert got[0]["tick"].tolist() == [61, 63, 65, 67] and got[0]["n"].tolist() == [3] * 4
    assert g.digest() == o.digest()
    g.close()


# ---- 9. ledger_now ----
def test_ledger_now_with_and_without_a_running_ledger(hiplib):
    _, entries, _, _, _, found = tl.deep_oracle()
    other = [e for e in sorted(found) if e not in entries][:20] + entries[:3]
    o = tl.maker(tl.DEEP_N, tl.DEEP_KW)()
    m = LedgerModel(o)
    g = serf_amd.create(tl.DEEP_N, **tl.DEEP_KW)
    for s in (o, g):
        tl.sc.apply_schedule(s, tl.sc.schedule(tl.DEEP_N, 40, rate=2.0, seed=524, max_member_subjects=40))
    m.step(30)
    g.step(30)
    for es in (entries, other, other[:1]):                                # without a running ledger
        gh, gr = g.ledger_now(es)
        wh, wr = m.now(es)
        assert words(gh).tolist() == words(wh).tolist() and words(gr).tolist() == words(wr).tolist()
    m.start(entries, 0, 1, 100)
    g.ledger_start(entries, 0, 1, 100)
    m.step(12)
    g.step(12)
    gh, gr = g.ledger_now(entries)                                        # the header and the records of the last sample
    oh, orr = g.ledger_now(other)                                         # entries other than the running ledger's
    wh, wr = m.now(other)
    assert words(oh).tolist() == words(wh).tolist() and words(orr).tolist() == words(wr).tolist() and wr["queued"].max() > 0
    m.step(6)
    g.step(6)
    got = g.ledger_read()
    assert g.ledger_count() == (18, 0)
    assert_same(got, m.read(), "a ledger that ledger_now looked past")   # the running ledger is untouched
    assert words(gh).tolist() == words(got[0][11]).tolist() and words(gr).tolist() == words(got[1][11]).tolist()
    assert words(oh)[[0, 1, 3, 4, 5, 6]].tolist() == words(got[0][11])[[0, 1, 3, 4, 5, 6]].tolist()
    assert g.digest() == o.digest()
    g.close()


# ---- 10. all five observers on one handle ----
def test_all_five_observers_on_one_handle(oracle, hiplib):
    """Each equals its own model, which does not know the others.  And without the oracle: the ledger's header words 3, 4 and 5
    equal the series' words at every common tick, and the reach of an event equals track_read's `last` for the same rumour at
    the last tick."""
    n, ticks, top_k = 4096, 160, 8
    kw = dict(tt.KW, flags=tt.KRANDOM)
    s = tt.script(n)
    # the events' Lamport times: a dry run (the trackers get theirs from sim.stats while the script runs)
    dry = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    lts = {}

    def dry_add(specs):
        for x in specs:
            if x.kind == _ffi.TRK_RUMOUR:
                lts[x.b] = int(x.ltime)
        return [0] * len(specs)
    tt.drive(dry, s, ticks, dry_add, dry.step)
    dry.close()
    events = [(_ffi.K_EVENT, key, lts[key]) for te, node, key in s["events"] if te < ticks]
    assert len(events) <= 48
    entries = events + [(_ffi.K_SUSPECT, c, 0) for c in s["crashed"]] + [(_ffi.K_DEAD, c, 0) for c in s["crashed"]]
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    tm, cm, rm, lm = TrackModel(o), CensusModel(o), RollModel(o), LedgerModel(o)
    sm = SeriesModel(o, lambda: (tm.evaluate(), cm.after_tick(o.tick - 1), rm.after_tick(o.tick - 1), lm.after_tick(o.tick - 1)))
    sm.start(0, 3, 1000)
    cm.start(0, 1, ticks, 64)
    rm.start(0, 1, ticks, top_k, _ffi.ROLL_BY_ACCUSED)
    lm.start(entries, 0, 1, ticks)
    mh = tt.drive(o, s, ticks, lambda specs: [tm.add(x) for x in specs], sm.step)
    want_trk = [tm.result(h) for h in mh]
    tl.inside_bounds(o)
    g = serf_amd.create(n, **kw)
    g.series_start(0, 3, 1000)
    g.census_start(0, 1, ticks, 64)
    g.roll_start(0, 1, ticks, top_k, _ffi.ROLL_BY_ACCUSED)
    g.ledger_start(entries, 0, 1, ticks)
    ids = tt.drive(g, s, ticks, g.track_add, g.step)
    trk = g.track_read(ids)
    tt.assert_same([r.as_dict() for r in trk], want_trk, "trackers next to the four samplers")
    ser = g.series_read()
    series_same(ser, sm.read(), "a series next to the others")
    census_same(g.census_read(), cm.read(), "a census next to the others")
    roll_same(g.roll_read(), rm.read(), "a roll next to the others")
    assert g.ledger_count() == lm.count() == (ticks, 0)
    lh, lr = g.ledger_read()
    assert_same((lh, lr), lm.read(), "a ledger next to the others")
    # without the oracle
    at = {int(t): i for i, t in enumerate(lh["tick"].tolist())}
    common = [at[int(t)] for t in ser["tick"].tolist()]
    assert len(common) == len(ser) > 50
    assert lh["queued"][common].tolist() == ser["queued"].sum(axis=1).tolist()
    assert lh["in_flight"][common].tolist() == ser["records"].sum(axis=1).tolist() and lh["packets"][common].tolist() == ser["packets"].tolist()
    assert lh["in_flight"].max() > 0 and lh["transmits"].max() > 0
    # (a tracker retires when everybody has the rumour and keeps that evaluation's count: the comparison is for those still open,
    # the events of the last ticks)
    n_member = len(ids) - len(events)
    still = [i for i in range(len(events)) if trk[n_member + i].as_dict()["state"] != 2]
    assert still, "no event tracker still open at the end"
    for i in still:
        assert int(lr["reach"][-1, i]) == trk[n_member + i].as_dict()["last"] < int(lh["running"][-1]), events[i]
    assert g.digest() == o.digest()
    g.close()


# ---- 11. errors ----
def test_errors_leave_everything_as_it_was(hiplib):
    n = 4096
    kw = tl.census_kw("krandomnodes")
    ok = [(_ffi.K_EVENT, 0x77, 3), (_ffi.K_LEAVE, 5, 2), (_ffi.K_SUSPECT, 9, 0)]
    sh = serf_amd.create(n, force_sharded=True, **kw)      # a shard has no ledger
    for call in (lambda: sh.ledger_start(ok), sh.ledger_count, lambda: sh.ledger_read(0, 0), sh.ledger_stop, lambda: sh.ledger_now(ok)):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    g = serf_amd.create(n, **kw)
    assert g.ledger_count() == (0, 0)
    for call in (lambda: g.ledger_read(0, 0), g.ledger_stop):           # no ledger yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    bad = [[], [(_ffi.K_JOIN, i, 1) for i in range(65)], [(0, 1, 1)], [(8, 1, 1)], [(_ffi.K_JOIN, n, 1)], [(_ffi.K_DEAD, n, 0)],
           [(_ffi.K_ALIVE, n + 5, 0)], [(_ffi.K_EVENT, 0, 1)], [(_ffi.K_QUERY, 0, 1)], [(_ffi.K_EVENT, 5, 1 << 48)],
           [(_ffi.K_LEAVE, 5, 1 << 48)], [(_ffi.K_SUSPECT, 5, 1 << 24)], [(_ffi.K_DEAD, 5, 1 << 24)],
           ok + [ok[1]], [ok[0], ok[0]]]
    for es in bad:
        with pytest.raises(_ffi.SimError) as ei:
            g.ledger_start(es, 0, 1, 8)
        assert ei.value.code == _ffi.EINVAL and g.ledger_count() == (0, 0), es
        with pytest.raises(_ffi.SimError) as ei:
            g.ledger_now(es)
        assert ei.value.code == _ffi.EINVAL, es
    for args in ((0, 0, 8), (0, 1, 0), (0, 1, _ffi.LEDGER_MAX_SAMPLES + 1)):
        with pytest.raises(_ffi.SimError) as ei:
            g.ledger_start(ok, *args)
        assert ei.value.code == _ffi.EINVAL and g.ledger_count() == (0, 0)
    start, now = g.lib.f["ledger_start"], g.lib.f["ledger_now"]
    out = np.zeros(HW + EW * 3, np.uint64)
    assert start(g.h, None, 3, 0, 1, 8) == _ffi.EINVAL and now(g.h, None, 3, out.ctypes.data) == _ffi.EINVAL
    assert now(g.h, _ffi.ledger_entries(ok), 3, None) == _ffi.EINVAL and start(None, _ffi.ledger_entries(ok), 3, 0, 1, 8) == _ffi.EINVAL
    assert not out.any() and g.ledger_count() == (0, 0)
    g.ledger_start([(_ffi.K_ALIVE, 5, 1 << 50)], 0, 1, 2)                 # an incarnation has no bound of the ledger's own
    g.ledger_stop()
    g.inject(1, _ffi.OP_CRASH, 9)
    g.leave(5)
    g.ledger_start(ok, 0, 1, 8)
    g.step(3)
    assert g.ledger_count() == (3, 0)
    before = g.ledger_read()
    assert before[0]["tick"].tolist() == [1, 2, 3] and before[1].shape == (3, 3)
    for first, cnt in ((0, 4), (3, 1), (4, 0)):                           # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.ledger_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL and g.ledger_count() == (3, 0)
    stride = HW + EW * 3
    fn, buf, got = g.lib.f["ledger_read"], np.zeros(2 * stride, np.uint64), _ffi.C.c_uint32(77)
    assert fn(g.h, 0, 3, buf.ctypes.data, buf.size, _ffi.C.byref(got)) == _ffi.EINVAL         # a buffer one sample short
    assert fn(g.h, 0, 2, None, buf.size, _ffi.C.byref(got)) == _ffi.EINVAL and fn(g.h, 0, 2, buf.ctypes.data, buf.size, None) == _ffi.EINVAL
    assert got.value == 77 and not buf.any()
    cnt, t, d = g.lib.f["ledger_count"], _ffi.C.c_uint32(77), _ffi.C.c_uint32(78)
    assert cnt(g.h, None, _ffi.C.byref(d)) == _ffi.EINVAL and cnt(g.h, _ffi.C.byref(t), None) == _ffi.EINVAL and cnt(None, _ffi.C.byref(t), _ffi.C.byref(d)) == _ffi.EINVAL
    assert (t.value, d.value) == (77, 78)
    for es in bad[:6]:                                                     # a refused start or now next to a running ledger
        with pytest.raises(_ffi.SimError):
            g.ledger_now(es)
    hdr, rec = g.ledger_now(ok)
    assert words(hdr).tolist() == words(before[0][-1]).tolist() and words(rec).tolist() == words(before[1][-1]).tolist()
    after = g.ledger_read()
    assert g.ledger_count() == (3, 0) and words(after[0]).tolist() == words(before[0]).tolist() and words(after[1]).tolist() == words(before[1]).tolist()
    g.close()
    t = serf_amd.create(256, fanout=3)                                   # inside a tick
    t.ledger_start(ok, 0, 1, 8)
    t.step(2)
    t.step_begin()
    for call in (lambda: t.ledger_start(ok), t.ledger_count, lambda: t.ledger_read(0, 1), t.ledger_stop, lambda: t.ledger_now(ok)):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                                   # a handle destroyed with a ledger running
    g.ledger_start(ok, 0, 1, 4)
    g.step(6)
    assert g.ledger_count() == (4, 2) and g.ledger_read()[0]["tick"].tolist() == [1, 2, 3, 4]
    g.close()
