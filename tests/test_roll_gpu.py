"""Observer roll (include/serf_sim_roll.h) on the GPU: every word of every header and of every listed node's record equals what
the reference model (tests/roll_model.py) computes from the dumps of the CPU oracle stepped one tick at a time.  The HIP handle
advances in long sim_step calls and is read once at the end; comparisons are exact, and in every test the digest equals the
oracle's.

roll_count_kernel has no pass loop: its grid is one workgroup per 256 nodes whatever the handle's size, so there is no cap and no
second-pass size to test."""
import functools

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_observer_shapes as shapes
from tests import test_roll as tr
from tests import test_track_gpu as tt
from tests.census_model import CensusModel
from tests.roll_model import RollModel
from tests.series_model import SeriesModel
from tests.test_census import census_drive, census_kw
from tests.test_census_gpu import assert_same as census_same
from tests.test_roll import ACCUSED, MISSED, STALE, TOP_K
from tests.test_series import scenario
from tests.test_series_gpu import assert_same as series_same
from tests.track_model import TrackModel

pytestmark = pytest.mark.gpu


def words(a):
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(a)))
    return a.view(np.uint64).reshape(a.shape + (a.dtype.itemsize // 8,))


def assert_same(got, want, what):
    """got, want: (headers, records) as roll_read returns them."""
    (gh, gr), (wh, wr) = got, want
    assert gh.dtype == _ffi.ROLL_HEADER_DTYPE and gr.dtype == _ffi.ROLL_NODE_DTYPE
    assert gh.shape == wh.shape and gr.shape == wr.shape, f"{what}: {gh.shape} / {gr.shape} samples, the model has {wh.shape} / {wr.shape}"
    g, w = words(gh), words(wh)
    bad = np.argwhere(g != w)
    msg = [f"sample {i} (tick word {int(w[i, 0])}) header word {j}: HIP {int(g[i, j])} != model {int(w[i, j])}" for i, j in bad[:12].tolist()]
    assert not len(bad), f"{what}: {len(bad)} header words differ\n" + "\n".join(msg)
    g, w = words(gr), words(wr)
    bad = np.argwhere(g != w)
    msg = [f"sample {i} (tick word {int(wh['tick'][i])}) record {r} word {j}: HIP {int(g[i, r, j])} (node {int(g[i, r, 0]) & 0xFFFFFFFF}) != "
           f"model {int(w[i, r, j])} (node {int(w[i, r, 0]) & 0xFFFFFFFF})" for i, r, j in bad[:12].tolist()]
    assert not len(bad), f"{what}: {len(bad)} record words differ\n" + "\n".join(msg)


def same_now(got, want, what):
    for g, w, part in zip(got, want, ("header", "top", "nodes")):
        bad = np.argwhere(words(g) != words(w))
        assert not len(bad), f"{what}: {part}: {len(bad)} words differ, the first at {bad[0].tolist()}: HIP {words(g)[tuple(bad[0])]} != model {words(w)[tuple(bad[0])]}"


# ---- 1. the census scenarios ----
@pytest.mark.parametrize("variant,by", [(v, STALE) for v in tr.VARIANTS] + [("lossy", ACCUSED), ("lossy", MISSED)])
def test_census_scenarios_4096_nodes_every_tick(hiplib, variant, by):
    run = tr.census_oracle(variant)
    tr.check_census_scenario(variant, run)
    o, reads, _ = run
    g = serf_amd.create(tr.N, **census_kw(variant))
    g.roll_start(0, 1, tr.TICKS, TOP_K, by)
    census_drive(g, scenario(tr.N), tr.TICKS, g.step)
    assert g.roll_count() == (tr.TICKS, 0)
    got = g.roll_read()            # read once, at the end
    assert_same(got, reads[by], f"{variant}, rank_by {by}")
    assert g.digest() == o.digest(), "a roll must not perturb the run"
    wh, wr = reads[by]
    assert_same(g.roll_read(10, 5), (wh[10:15], wr[10:15]), variant + " [10, 15)")   # parts of the buffer
    assert_same(g.roll_read(tr.TICKS - 1, 1), (wh[-1:], wr[-1:]), variant + " the last one")
    h, r = g.roll_read(tr.TICKS, 0)
    assert len(h) == 0 and len(r) == 0


# ---- 2. busy ----
def test_busy_ties_across_workgroups(hiplib):
    run = tr.busy_oracle()
    tr.check_busy(run)
    o, want, _ = run
    g = serf_amd.create(tr.N, **tr.BUSY_KW)
    g.roll_start(0, tr.BUSY_PERIOD, 100, TOP_K, STALE)
    tr.busy_script(g, g.step)      # one call
    assert g.roll_count() == (tr.BUSY_TICKS // tr.BUSY_PERIOD, 0)
    assert_same(g.roll_read(), want, "busy")
    assert g.digest() == o.digest()


# ---- 3. cold join ----
def test_cold_join_one_wave_dense(hiplib):
    run = tr.cold_oracle()
    tr.check_cold(run)
    o, want = run
    g = serf_amd.create(tr.COLD_N, **tr.COLD_KW)
    g.roll_start(0, 1, tr.COLD_TICKS, tr.COLD_TOP, STALE)
    tr.cold_script(g, g.step)
    assert g.roll_count() == (tr.COLD_TICKS, 0)
    assert_same(g.roll_read(), want, "cold join")
    assert g.digest() == o.digest()


# ---- 4. eight nodes ----
def test_eight_nodes(oracle, hiplib):
    """tests/test_census_gpu.py's script: a partial wave, a liveness bitmap of one partial word."""
    n, ticks = 8, 24
    kw = dict(fanout=3, event_ring=64, query_ring=64)

    def run(sim, step):
        sim.inject(3, _ffi.OP_CRASH, 6)
        step(5)
        sim.leave(2)
        step(ticks - 5)
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = RollModel(o)
    m.start(0, 1, ticks, n, MISSED)
    run(o, m.step)
    g = serf_amd.create(n, **kw)
    g.roll_start(0, 1, ticks, n, MISSED)
    run(g, g.step)
    wh, wr = m.read()
    tr.inside_bounds(o)
    assert (wh["running"][3:] == n - 1).all() and (wh["stale_alive_sum"][3:] == n - 1).all()   # (no SWIM layer: nobody notices)
    assert ((wh["listed"][3:] & 0xFFFFFFFF) == n - 1).all() and wh["stale_max"].max() > 0
    assert_same(g.roll_read(), (wh, wr), "8 nodes")
    assert g.digest() == o.digest()


# ---- 5. ragged and idle sizes ----
def no_tracker(spec):
    return 0


@functools.lru_cache(maxsize=None)
def ragged_oracle(n):
    o = _ffi.Sim(shapes.load_oracle(), _ffi.make_config(n, **shapes.ragged_kw(n, "krandomnodes")))
    m = RollModel(o)
    m.start(0, 1, shapes.RAGGED_TICKS, TOP_K, STALE)
    shapes.ragged_script(o, n, no_tracker, m.step)
    return o, m.read()


@pytest.mark.parametrize("n", shapes.RAGGED_SIZES)
def test_ragged_sizes(hiplib, n):
    o, want = ragged_oracle(n)
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    running = want[0]["running"].tolist()
    assert running[0] == n and running[-1] == max(n - 2, 1) and (n < 3 or want[0]["stale_max"].max() > 0)
    g = serf_amd.create(n, **shapes.ragged_kw(n, "krandomnodes"))
    g.roll_start(0, 1, shapes.RAGGED_TICKS, TOP_K, STALE)
    shapes.ragged_script(g, n, no_tracker, g.step)
    assert g.roll_count() == (shapes.RAGGED_TICKS, 0)
    assert_same(g.roll_read(), want, f"ragged({n})")
    assert g.digest() == o.digest()


@pytest.mark.parametrize("n", shapes.IDLE_SIZES)
def test_nobody_runs(oracle, hiplib, n):
    kw = dict(shapes.KW, view_slots=0, flags=shapes.FANOUTS["krandomnodes"])
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = RollModel(o)
    m.start(0, 1, shapes.IDLE_TICKS, TOP_K, ACCUSED)
    shapes.idle_script(o, n, no_tracker, m.step)
    wh, wr = m.read()
    tr.inside_bounds(o)
    idle = words(wh)[shapes.IDLE_CRASH:]
    assert (wh["running"][shapes.IDLE_CRASH:] == 0).all() and (idle[:, 2] == n).all() and (idle[:, 3] == ACCUSED << 32).all()
    assert not idle[:, 1].any() and not idle[:, 4:].any()          # every word but 0, 2 and 3
    g = serf_amd.create(n, **kw)
    g.roll_start(0, 1, shapes.IDLE_TICKS, TOP_K, ACCUSED)
    shapes.idle_script(g, n, no_tracker, g.step)
    assert_same(g.roll_read(), (wh, wr), f"nobody runs ({n})")
    assert g.digest() == o.digest()


# ---- 6. a large size ----
def test_69700_nodes(hiplib):
    """tests/test_census_gpu.py's run of that size: 273 workgroups, the last one of 68 nodes — a whole wave and four lanes — and a
    last word of the liveness bitmap that is partial (69 700 = 2 178 * 32 + 4)."""
    n, ticks, period, over = 69700, 120, 5, dict(view_slots=16)
    o = _ffi.Sim(shapes.load_oracle(), _ffi.make_config(n, **dict(census_kw("krandomnodes"), **over)))
    m = RollModel(o)
    m.start(0, period, 1000, TOP_K, STALE)
    census_drive(o, scenario(n), ticks, m.step)
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    wh, wr = m.read()
    # (at this size nobody is declared Failed within 120 ticks: the accusations here are suspicions)
    assert wh["stale_max"].max() >= 2 and wh["holders_stale_alive"].max() > 0 and wh["accusers_suspect"].max() > 0 and wh["subjects"].max() >= 8
    g = serf_amd.create(n, **dict(census_kw("krandomnodes"), **over))
    g.roll_start(0, period, 1000, TOP_K, STALE)
    census_drive(g, scenario(n), ticks, g.step)
    assert g.roll_count() == m.count() == (ticks // period, 0)
    assert_same(g.roll_read(), (wh, wr), f"{n} nodes")
    assert g.digest() == o.digest()


# ---- 7. slots come and go ----
def test_slots_come_and_go_during_one_long_step(hiplib):
    run = tr.slots_oracle()
    tr.check_slots(run)
    o, want, _ = run
    g = serf_amd.create(tr.N, **tr.SLOTS_KW)
    g.roll_start(0, 1, tr.SLOTS_TICKS, TOP_K, STALE)
    tr.slots_script(g, g.step)     # every operation injected up front, one call
    assert g.roll_count() == (tr.SLOTS_TICKS, 0)
    assert_same(g.roll_read(), want, "slots come and go")
    assert g.digest() == o.digest()


# ---- 7b. more than one chunk of slots ----
def test_the_chunk_is_the_sources():
    """tests/test_roll.ROLL_CHUNK mirrors this line; a change there has to move the sizes of the two tests below."""
    import os
    src = open(os.path.join(tr.ROOT, "serf_amd", "csrc", "serf_sim_roll.inc")).read()
    assert f"#define ROLL_CHUNK {tr.ROLL_CHUNK}u " in src and "for (u32 a0 = 0; a0 < p.bound; a0 += ROLL_CHUNK)" in src


def test_dense_600_nodes_three_chunks(hiplib):
    """2 * ROLL_CHUNK + 88 subjects: the LDS lists are written three times, the last list is short of a batch's multiple."""
    run = tr.dense_oracle()
    tr.check_dense(run)
    o, want = run
    g = serf_amd.create(tr.DENSE_N, **tr.DENSE_KW)
    g.roll_start(0, tr.DENSE_PERIOD, 100, TOP_K, STALE)
    tr.dense_script(g, g.step)
    assert g.roll_count() == (tr.DENSE_TICKS // tr.DENSE_PERIOD, 0)
    assert_same(g.roll_read(), want, "dense, three chunks")
    same_now(g.roll_now(64, ACCUSED, nodes=True), RollModel(o).now(64, ACCUSED, nodes=True), "roll_now over three chunks")
    assert g.digest() == o.digest()


def test_subjects_grow_into_a_second_chunk(hiplib):
    """The subjects pass ROLL_CHUNK while one sim_step(600) runs: a full first list, then second lists of 1 to 35 slots."""
    run = tr.grow_oracle()
    tr.check_grow(run)
    o, want = run
    g = serf_amd.create(tr.GROW_N, **tr.GROW_KW)
    g.roll_start(0, tr.GROW_PERIOD, 100, TOP_K, STALE)
    tr.grow_script(g, g.step)      # one call
    assert g.roll_count() == (tr.GROW_TICKS // tr.GROW_PERIOD, 0)
    assert_same(g.roll_read(), want, "subjects grow into a second chunk")
    assert g.digest() == o.digest()


# ---- 8. period, first tick, capacity, restart ----
def test_period_first_tick_capacity_and_restart(oracle, hiplib):
    """Period 7 from a first tick in the future, a buffer three short of what the run would fill; a second roll after
    sim_roll_stop begins at sample 0, with another top_k and rank_by."""
    n, ticks, first, period = 4096, 200, 13, 7
    due = len(range(first, ticks, period))
    kw = census_kw("lossy")
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = RollModel(o)
    m.start(first, period, due - 3, TOP_K, STALE)
    census_drive(o, scenario(n), ticks, m.step)
    g = serf_amd.create(n, **kw)
    g.roll_start(first, period, due - 3, TOP_K, STALE)
    census_drive(g, scenario(n), ticks, g.step)
    assert g.roll_count() == m.count() == (due - 3, 3)
    got = g.roll_read()
    assert_same(got, m.read(), "period 7")
    assert got[0]["tick"].tolist() == [t + 1 for t in range(first, ticks, period)][:due - 3]
    with pytest.raises(_ffi.SimError) as ei:
        g.roll_start(0, 1, 8, 4, STALE)        # one roll at a time
    assert ei.value.code == _ffi.ESTATE and g.roll_count() == (due - 3, 3)
    assert_same(g.roll_read(), m.read(), "after the refused start")
    g.roll_stop()
    m.stop()
    assert g.roll_count() == (0, 0)
    with pytest.raises(_ffi.SimError) as ei:
        g.roll_read(0, 0)
    assert ei.value.code == _ffi.ESTATE
    g.roll_start(5, 2, 4, 3, ACCUSED)          # a first tick that has passed: now (tick 200)
    m.start(5, 2, 4, 3, ACCUSED)
    g.step(9)
    m.step(9)
    assert g.roll_count() == m.count() == (4, 1)
    got = g.roll_read()
    assert_same(got, m.read(), "second roll")
    tr.inside_bounds(o)
    assert got[0]["tick"].tolist() == [201, 203, 205, 207] and got[1].shape == (4, 3)
    assert ((got[0]["listed"] & 0xFFFFFFFF) > 0).all()
    assert g.digest() == o.digest()


# ---- 9. roll_now ----
def test_roll_now_with_and_without_a_running_roll(hiplib):
    """At 4 096 nodes, after the busy script: every node's record equals the model's, stopped nodes are zero but the id, and the
    header equals the last sample's."""
    o, (wh, wr), _ = tr.busy_oracle()
    m = RollModel(o)
    g = serf_amd.create(tr.N, **tr.BUSY_KW)
    g.roll_start(0, tr.BUSY_PERIOD, 100, TOP_K, STALE)
    tr.busy_script(g, g.step)                                       # (the last sampled tick is 76: three more follow it)
    g2 = serf_amd.create(tr.N, **tr.BUSY_KW)
    g2.roll_start(0, 1, 100, TOP_K, STALE)
    tr.busy_script(g2, g2.step)
    for by, k in ((STALE, TOP_K), (ACCUSED, 64), (MISSED, 1)):
        want = m.now(k, by, nodes=True)
        same_now(g.roll_now(k, by, nodes=True), want, f"roll_now({k}, {by}, nodes) next to a running roll")
        same_now(g.roll_now(k, by), want[:2], f"roll_now({k}, {by})")
    hdr, top, every = g.roll_now(TOP_K, STALE, nodes=True)
    stopped = (every["id"] >> 32) == 0
    assert 0 < stopped.sum() < tr.N and not words(every)[stopped][:, 1:].any()
    assert (every["id"] & 0xFFFFFFFF).tolist() == list(range(tr.N)) and int(hdr["running"]) == int((~stopped).sum())
    assert every["stale"].max() == hdr["stale_max"] and int(every["lag"].sum()) == int(hdr["lag_sum"])
    (lh,), (lr,) = g2.roll_read(tr.BUSY_TICKS - 1, 1)               # the last sample of a roll behind every tick
    assert words(lh).tolist() == words(hdr).tolist() and words(lr).tolist() == words(top).tolist()
    assert g.roll_count() == (tr.BUSY_TICKS // tr.BUSY_PERIOD, 0)   # roll_now does not touch the running roll
    assert_same(g.roll_read(), (wh, wr), "the running roll after roll_now")
    g.roll_stop()
    same_now(g.roll_now(TOP_K, STALE, nodes=True), (hdr, top, every), "roll_now without a roll")
    assert g.digest() == o.digest() == g2.digest()


# ---- 10. roll, census, series and trackers on one handle ----
def test_roll_census_series_and_trackers_on_one_handle(oracle, hiplib):
    """Each equals its own model, which does not know the others.  And without the oracle: the roll's header words 9, 11 and 13
    — pairs counted per observer — equal the census header's words 6, 8 and 10 — the same pairs counted per subject — at every
    sampled tick."""
    n, ticks = 4096, 160
    kw = dict(tt.KW, flags=tt.KRANDOM)
    s = tt.script(n)
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    tm, cm, rm = TrackModel(o), CensusModel(o), RollModel(o)
    sm = SeriesModel(o, lambda: (tm.evaluate(), cm.after_tick(o.tick - 1), rm.after_tick(o.tick - 1)))
    sm.start(0, 3, 1000)
    cm.start(0, 1, ticks, 64)
    rm.start(0, 1, ticks, TOP_K, ACCUSED)
    mh = tt.drive(o, s, ticks, lambda specs: [tm.add(x) for x in specs], sm.step)
    want_trk = [tm.result(h) for h in mh]
    tr.inside_bounds(o)
    g = serf_amd.create(n, **kw)
    g.series_start(0, 3, 1000)
    g.census_start(0, 1, ticks, 64)
    g.roll_start(0, 1, ticks, TOP_K, ACCUSED)
    ids = tt.drive(g, s, ticks, g.track_add, g.step)
    tt.assert_same([r.as_dict() for r in g.track_read(ids)], want_trk, "trackers next to a series, a census and a roll")
    series_same(g.series_read(), sm.read(), "a series next to the others")
    census_same(g.census_read(), cm.read(), "a census next to the others")
    assert g.roll_count() == rm.count() == (ticks, 0)
    rh, rr = g.roll_read()
    assert_same((rh, rr), rm.read(), "a roll next to the others")
    ch = g.census_read()[0]
    assert rh["tick"].tolist() == ch["tick"].tolist()
    for a, b in (("false_failed_sum", "false_failed_pairs"), ("suspects_sum", "suspected_running_pairs"), ("stale_alive_sum", "stopped_alive_pairs")):
        assert rh[a].tolist() == ch[b].tolist(), (a, b)
    # (nobody comes back in this script and no running member is suspected: the pairs that occur are stopped members held Alive; the
    # census scenarios and tests/test_roll.py cover the other two words against the census model)
    assert rh["stale_alive_sum"].max() > 0
    assert g.digest() == o.digest()


# ---- 11. errors ----
def test_errors_leave_everything_as_it_was(hiplib):
    n = 4096
    kw = census_kw("krandomnodes")
    sh = serf_amd.create(n, force_sharded=True, **kw)      # a shard has no roll
    for call in (lambda: sh.roll_start(0, 1, 8, 4), sh.roll_count, lambda: sh.roll_read(0, 0), sh.roll_stop, sh.roll_now):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    g = serf_amd.create(n, **kw)
    assert g.roll_count() == (0, 0)
    for call in (lambda: g.roll_read(0, 0), g.roll_stop):               # no roll yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    for args in ((0, 0, 8, 4, STALE), (0, 1, 0, 4, STALE), (0, 1, _ffi.ROLL_MAX_SAMPLES + 1, 4, STALE), (0, 1, 8, 0, STALE),
                 (0, 1, 8, _ffi.ROLL_TOP_MAX + 1, STALE), (0, 1, 8, 4, 3), (0, 1, 8, 4, 0xFFFFFFFF)):
        with pytest.raises(_ffi.SimError) as ei:
            g.roll_start(*args)
        assert ei.value.code == _ffi.EINVAL and g.roll_count() == (0, 0)
    g.inject(1, _ffi.OP_CRASH, 9)
    g.leave(5)
    g.roll_start(0, 1, 8, 4, MISSED)
    g.step(3)
    assert g.roll_count() == (3, 0)
    before = g.roll_read()
    assert before[0]["subjects"].tolist() == [1, 2, 2] and before[1].shape == (3, 4)
    assert (before[0]["listed"][1:] & 0xFFFFFFFF).tolist() == [4, 4]       # everybody still holds the crashed node Alive
    for first, cnt in ((0, 4), (3, 1), (4, 0)):                           # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.roll_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL and g.roll_count() == (3, 0)
    stride = 32 + 8 * 4
    fn, out, got = g.lib.f["roll_read"], np.zeros(2 * stride, np.uint64), _ffi.C.c_uint32(77)
    assert fn(g.h, 0, 3, out.ctypes.data, out.size, _ffi.C.byref(got)) == _ffi.EINVAL         # a buffer one sample short
    assert fn(g.h, 0, 2, None, out.size, _ffi.C.byref(got)) == _ffi.EINVAL and fn(g.h, 0, 2, out.ctypes.data, out.size, None) == _ffi.EINVAL
    assert got.value == 77 and not out.any()
    cnt, t, d = g.lib.f["roll_count"], _ffi.C.c_uint32(77), _ffi.C.c_uint32(78)
    assert cnt(g.h, None, _ffi.C.byref(d)) == _ffi.EINVAL and cnt(g.h, _ffi.C.byref(t), None) == _ffi.EINVAL and cnt(None, _ffi.C.byref(t), _ffi.C.byref(d)) == _ffi.EINVAL
    assert (t.value, d.value) == (77, 78)
    now = g.lib.f["roll_now"]
    hdr, top = np.zeros(1, _ffi.ROLL_HEADER_DTYPE), np.zeros(4, _ffi.ROLL_NODE_DTYPE)
    for args in ((0, STALE, hdr.ctypes.data, top.ctypes.data, None), (65, STALE, hdr.ctypes.data, top.ctypes.data, None),
                 (4, 3, hdr.ctypes.data, top.ctypes.data, None), (4, STALE, None, top.ctypes.data, None), (4, STALE, hdr.ctypes.data, None, None)):
        assert now(g.h, *args) == _ffi.EINVAL
    assert not words(hdr).any() and not words(top).any()
    assert now(g.h, 4, MISSED, hdr.ctypes.data, top.ctypes.data, None) == 0
    assert words(hdr[0]).tolist() == words(before[0][-1]).tolist() and words(top).tolist() == words(before[1][-1]).tolist()
    after = g.roll_read()
    assert g.roll_count() == (3, 0) and words(after[0]).tolist() == words(before[0]).tolist() and words(after[1]).tolist() == words(before[1]).tolist()
    g.close()
    t = serf_amd.create(256, fanout=3)                                   # inside a tick
    t.roll_start(0, 1, 8, 4)
    t.step(2)
    t.step_begin()
    for call in (lambda: t.roll_start(0, 1, 8, 4), t.roll_count, lambda: t.roll_read(0, 1), t.roll_stop, t.roll_now):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                                   # a handle destroyed with a roll running
    g.roll_start(0, 1, 4, 64)
    g.step(6)
    assert g.roll_count() == (4, 2) and g.roll_read()[0]["tick"].tolist() == [1, 2, 3, 4]
    g.close()
