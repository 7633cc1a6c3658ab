"""Membership census (include/serf_sim_census.h) on the GPU: every word of every header and of every subject's record equals
what the reference model (tests/census_model.py) computes from the dumps of the CPU oracle stepped one tick at a time.  The
HIP handle is driven in one sim_step per stretch between two injections and read once at the end; comparisons are exact."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_track_gpu as tt
from tests.census_model import CensusModel
from tests.series_model import SeriesModel
from tests.test_census import MAX_SUBJECTS, VARIANTS, census_drive, census_kw, check_nontrivial, oracle_run
from tests.test_series import scenario
from tests.test_series_gpu import assert_same as series_same
from tests.track_model import TrackModel

pytestmark = pytest.mark.gpu

CEN_SEG = 8192          # nodes a workgroup of census_count_kernel covers (serf_amd/csrc/serf_sim_census.inc)


def words(a):
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(a)))
    return a.view(np.uint64).reshape(a.shape + (_ffi.CENSUS_WORDS,))


def assert_same(got, want, what):
    """got, want: (headers, records) as census_read returns them."""
    (gh, gr), (wh, wr) = got, want
    assert gh.dtype == _ffi.CENSUS_HEADER_DTYPE and gr.dtype == _ffi.CENSUS_SUBJECT_DTYPE
    assert gh.shape == wh.shape and gr.shape == wr.shape, f"{what}: {gh.shape} / {gr.shape} samples, the model has {wh.shape} / {wr.shape}"
    g, w = words(gh), words(wh)
    bad = np.argwhere(g != w)
    msg = [f"sample {i} (tick word {int(w[i, 0])}) header word {j}: HIP {int(g[i, j])} != model {int(w[i, j])}" for i, j in bad[:12].tolist()]
    assert not len(bad), f"{what}: {len(bad)} header words differ\n" + "\n".join(msg)
    g, w = words(gr), words(wr)
    bad = np.argwhere(g != w)
    msg = [f"sample {i} (tick word {int(wh['tick'][i])}) record {r} (subject {int(w[i, r, 0]) & 0xFFFFFFFF}) word {j}: HIP {int(g[i, r, j])} != "
           f"model {int(w[i, r, j])}" for i, r, j in bad[:12].tolist()]
    assert not len(bad), f"{what}: {len(bad)} record words differ\n" + "\n".join(msg)


def hip_run(variant, n, ticks, first=0, period=1, capacity=None, max_subjects=MAX_SUBJECTS, **over):
    g = serf_amd.create(n, **dict(census_kw(variant), **over))
    g.census_start(first, period, capacity or ticks, max_subjects)
    census_drive(g, scenario(n), ticks, g.step)
    return g


@pytest.mark.parametrize("variant", VARIANTS)
def test_parity_4096_nodes_every_tick(hiplib, variant):
    n, ticks = 4096, 200
    o, m, wh, wr = oracle_run(variant)
    check_nontrivial(o, wh, wr, variant)
    g = hip_run(variant, n, ticks)
    assert g.census_count() == m.count() == (ticks, 0)
    got = g.census_read()          # read once, at the end
    assert_same(got, (wh, wr), variant)
    assert got[0]["tick"].tolist() == list(range(1, ticks + 1))
    assert g.digest() == o.digest(), "a census must not perturb the run"
    # parts of the buffer
    assert_same(g.census_read(10, 5), (wh[10:15], wr[10:15]), variant + " [10, 15)")
    assert_same(g.census_read(ticks - 1, 1), (wh[-1:], wr[-1:]), variant + " the last one")
    h, r = g.census_read(ticks, 0)
    assert len(h) == 0 and len(r) == 0


def test_dense_and_truncated(oracle, hiplib):
    """256 nodes, every node a subject (slot == id), 40 records of 256: the header's words 4 - 11 still cover all subjects —
    the victims (ids 100, 200) and the member that leaves (150) lie beyond the records that are kept."""
    n, ticks, ms = 256, 80, 40
    kw = dict(fanout=3, probe_interval=5, loss=0.02, event_ring=64, query_ring=64)

    def run(sim, step):
        sim.inject(4, _ffi.OP_CRASH, 100)
        sim.inject(9, _ffi.OP_CRASH, 200)
        step(12)
        sim.leave(150)
        step(ticks - 12)
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = CensusModel(o)
    m.start(0, 1, ticks, ms)
    run(o, m.step)
    g = serf_amd.create(n, **kw)
    g.census_start(0, 1, ticks, ms)
    run(g, g.step)
    wh, wr = m.read()
    assert (wh["subjects"] == n).all() and (wh["stored"] == ms).all() and wr.shape == (ticks, ms)
    assert wh["stopped_alive"].max() == 2 and wh["detected"].max() >= 1 and wh["settled"].min() <= n - 2   # from beyond record 40
    assert_same(g.census_read(), (wh, wr), "dense, truncated")
    # census_now: the last sample again (the tick has not moved), next to the running census and with any cap
    for cap in (ms, n + 44, 1, 0):
        h, r = g.census_now(cap)
        mh, mr = m.now(cap)
        assert words(h).tolist() == words(mh).tolist() and words(r).tolist() == words(mr).tolist(), f"census_now({cap})"
        assert len(r) == min(cap, n)
    h, r = g.census_now(ms)
    assert words(h).tolist() == words(wh[-1]).tolist() and words(r).tolist() == words(wr[-1]).tolist()
    assert g.census_count() == (ticks, 0)
    g.census_stop()
    h2, r2 = g.census_now(ms)                                      # and without one
    assert words(h2).tolist() == words(h).tolist() and words(r2).tolist() == words(r).tolist()
    assert g.digest() == o.digest()


def test_eight_nodes(oracle, hiplib):
    """A node count that is no multiple of 64: 8, the smallest one other GPU tests create (tests/test_host_paths_gpu.py).
    One workgroup per slot, 8 of its 256 lanes with an entry, a liveness bitmap of one partial word."""
    n, ticks = 8, 24
    kw = dict(fanout=3, event_ring=64, query_ring=64)

    def run(sim, step):
        sim.inject(3, _ffi.OP_CRASH, 6)
        step(5)
        sim.leave(2)
        step(ticks - 5)
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = CensusModel(o)
    m.start(0, 1, ticks, n)
    run(o, m.step)
    g = serf_amd.create(n, **kw)
    g.census_start(0, 1, ticks, n)
    run(g, g.step)
    wh, wr = m.read()
    assert (wh["running"][3:] == n - 1).all() and (wh["stopped_alive_pairs"][3:] == n - 1).all()   # (no SWIM layer: nobody notices)
    assert wr["status"][:, 2, _ffi.STATUS_LEAVING].tolist()[4:9] == [0, 1, 4, 6, 7] and wh["settled"].min() == n - 1
    assert_same(g.census_read(), (wh, wr), "8 nodes")
    assert g.digest() == o.digest()


@pytest.mark.parametrize("n", [65536, 8 * CEN_SEG + 4164])
def test_slots_that_span_segments(hiplib, n):
    """65 536 nodes: a slot's plane is 8 segments of CEN_SEG = 8 192 nodes, the fold has 8 partial records to combine.
    69 700 = 8 * 8 192 + 4 164 nodes: a ninth segment that is partial, whose last pass over the lanes (4 164 = 16 * 256 + 68),
    last wave (68 = 64 + 4) and last word of the liveness bitmap (69 700 = 2 178 * 32 + 4) are partial too."""
    ticks = 120
    over = dict(view_slots=16)
    o, m, wh, wr = oracle_run("krandomnodes", n, ticks, 0, 5, 1000, 16, tuple(over.items()))
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    assert wh["stopped_alive"].max() > 0 and (wr["inc_min"] < wr["inc_max"]).any() and (wr["ltime_min"] < wr["ltime_max"]).any()
    assert wh["subjects"].max() >= 8 and (wh["settled"] < wh["subjects"]).any()
    g = hip_run("krandomnodes", n, ticks, 0, 5, 1000, 16, **over)
    assert g.census_count() == m.count() == (ticks // 5, 0)
    assert_same(g.census_read(), (wh, wr), f"{n} nodes")
    assert g.digest() == o.digest()


def test_slots_come_and_go_during_one_long_step(oracle, hiplib):
    """16 view slots, a recycling pass every 20 ticks, every operation injected up front and ONE sim_step(170): slots are
    handed out and given back while the host runs ahead of the device; which slots hold a subject the census asks the device."""
    n, ticks = 4096, 170
    kw = dict(fanout=4, view_slots=16, event_ring=64, query_ring=64, probe_interval=5, loss=0.01, push_pull_interval=150,
              join_sync=True, recycle_interval=20, flags=tt.KRANDOM)

    def ops(sim):
        sim.inject(5, _ffi.OP_CRASH, 300)
        sim.inject(40, _ffi.OP_REVIVE, 300)
        sim.inject(12, _ffi.OP_LEAVE, 100)
        sim.inject(50, _ffi.OP_CRASH, 2000)
        sim.inject(90, _ffi.OP_CRASH, 7)
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = CensusModel(o)
    m.start(0, 1, ticks, 16)
    ops(o)
    m.step(ticks)
    wh, wr = m.read()
    cs = o.cluster_stats()
    d = np.diff(wh["subjects"].astype(np.int64))
    assert cs["slots_recycled"] > 0 and (d > 0).any() and (d < 0).any(), "the allocated set was to grow and to shrink"
    ids = [set((r["id"][:int(h["stored"])] >> 32).tolist()) for h, r in zip(wh, wr)]
    assert any(sorted(s) != list(range(len(s))) for s in ids), "no sample with a free slot below an allocated one"
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    g = serf_amd.create(n, **kw)
    g.census_start(0, 1, ticks, 16)
    ops(g)
    g.step(ticks)                  # one call
    assert g.census_count() == (ticks, 0)
    assert_same(g.census_read(), (wh, wr), "slots come and go")
    assert g.digest() == o.digest()


def test_period_first_tick_capacity_and_restart(oracle, hiplib):
    """Period 7 from a first tick in the future, a buffer three short of what the run would fill; a second census after
    sim_census_stop begins at sample 0 (with another max_subjects)."""
    n, ticks, first, period = 4096, 200, 13, 7
    due = len(range(first, ticks, period))
    kw = census_kw("krandomnodes")
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = CensusModel(o)
    m.start(first, period, due - 3, MAX_SUBJECTS)
    census_drive(o, scenario(n), ticks, m.step)
    g = hip_run("krandomnodes", n, ticks, first, period, due - 3)
    assert g.census_count() == m.count() == (due - 3, 3)
    got = g.census_read()
    assert_same(got, m.read(), "period 7")
    assert got[0]["tick"].tolist() == [t + 1 for t in range(first, ticks, period)][:due - 3]
    with pytest.raises(_ffi.SimError) as ei:
        g.census_start(0, 1, 8, 4)             # one census at a time
    assert ei.value.code == _ffi.ESTATE and g.census_count() == (due - 3, 3)
    assert_same(g.census_read(), m.read(), "after the refused start")
    g.census_stop()
    m.stop()
    assert g.census_count() == (0, 0)
    with pytest.raises(_ffi.SimError) as ei:
        g.census_read(0, 0)
    assert ei.value.code == _ffi.ESTATE
    g.census_start(5, 2, 4, 3)                 # a first tick that has passed: now (tick 200)
    m.start(5, 2, 4, 3)
    g.step(9)
    m.step(9)
    assert g.census_count() == m.count() == (4, 1)
    got = g.census_read()
    assert_same(got, m.read(), "second census")
    assert got[0]["tick"].tolist() == [201, 203, 205, 207] and got[1].shape == (4, 3)
    assert g.digest() == o.digest()


def test_census_series_and_trackers_on_one_handle(oracle, hiplib):
    """tests/test_track_gpu.py's trackers, a series of period 3 and a census behind every tick together: each equals its own
    model, which does not know the others.  And without the oracle, two routes on the GPU to one number: a MEMBER tracker that
    asks for one status (or one memberlist state) of a subject counts what one bin of the subject's census record holds — its
    `last` / `last_up`, read at the end of a stretch, against the sample of the stretch's last tick."""
    n, ticks = 4096, 160
    kw = dict(tt.KW, flags=tt.KRANDOM)
    s = tt.script(n)
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    tm = TrackModel(o)
    cm = CensusModel(o)
    sm = SeriesModel(o, lambda: (tm.evaluate(), cm.after_tick(o.tick - 1)))
    sm.start(0, 3, 1000)
    cm.start(0, 1, ticks, MAX_SUBJECTS)
    mh = tt.drive(o, s, ticks, lambda specs: [tm.add(x) for x in specs], sm.step)
    want_trk = [tm.result(h) for h in mh]

    g = serf_amd.create(n, **kw)
    g.series_start(0, 3, 1000)
    g.census_start(0, 1, ticks, MAX_SUBJECTS)
    one_bin = []                         # (tracker id, subject, field, bin): GPU only, the model does not know them
    for t, c in zip(s["crash_at"], s["crashed"]):
        for field, b, spec in (("status", _ffi.STATUS_FAILED, _ffi.member_tracker(c, tt.FAILED, start=t)),
                               ("swim", _ffi.SWIM_SUSPECT, _ffi.member_tracker(c, 0, 1 << _ffi.SWIM_SUSPECT, start=t)),
                               ("swim", _ffi.SWIM_DEAD, _ffi.member_tracker(c, 0, 1 << _ffi.SWIM_DEAD, start=t))):
            one_bin.append((g.track_add([spec])[0], c, field, b))
    checked = []

    def two_routes():
        taken = g.census_count()[0]
        if not taken:
            return
        (h,), (r,) = g.census_read(taken - 1, 1)
        assert int(h["tick"]) == g.tick
        by_subject = {int(x["id"]) & 0xFFFFFFFF: x for x in r[:int(h["stored"])]}
        for (i, c, field, b), res in zip(one_bin, g.track_read([x[0] for x in one_bin])):
            if res.state != 1 or not res.evaluated or c not in by_subject:
                continue                 # (not started, retired at an earlier tick, or no slot yet)
            assert (res.last, res.last_up) == (int(by_subject[c][field][b]), int(h["running"])), f"tick {g.tick} subject {c} {field}[{b}]"
            checked.append(res.last)
    ids = tt.drive(g, s, ticks, g.track_add, g.step, on_stretch=two_routes)
    assert len(checked) >= 100 and sum(1 for x in checked if x) >= 20, "the two routes were to meet often, on counts that are not 0"
    tt.assert_same([r.as_dict() for r in g.track_read(ids)], want_trk, "trackers next to a series and a census")
    assert g.series_count() == sm.count() == (len(range(0, ticks, 3)), 0)
    series_same(g.series_read(), sm.read(), "a series next to trackers and a census")
    assert g.census_count() == cm.count() == (ticks, 0)
    assert_same(g.census_read(), cm.read(), "a census next to trackers and a series")
    assert g.digest() == o.digest()


def test_errors_leave_everything_as_it_was(hiplib):
    n = 4096
    kw = census_kw("krandomnodes")
    sh = serf_amd.create(n, force_sharded=True, **kw)      # a shard has no census
    for call in (lambda: sh.census_start(0, 1, 8, 4), sh.census_count, lambda: sh.census_read(0, 0), sh.census_stop, sh.census_now):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    g = serf_amd.create(n, **kw)
    assert g.census_count() == (0, 0)
    for call in (lambda: g.census_read(0, 0), g.census_stop):             # no census yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    for args in ((0, 0, 8, 4), (0, 1, 0, 4), (0, 1, _ffi.CENSUS_MAX_SAMPLES + 1, 4), (0, 1, 8, 0)):
        with pytest.raises(_ffi.SimError) as ei:
            g.census_start(*args)
        assert ei.value.code == _ffi.EINVAL and g.census_count() == (0, 0)
    g.inject(1, _ffi.OP_CRASH, 9)
    g.leave(5)
    g.census_start(0, 1, 8, 4)
    g.step(3)
    assert g.census_count() == (3, 0)
    before = g.census_read()
    assert before[0]["subjects"].tolist() == [1, 2, 2] and before[1].shape == (3, 4)
    for first, cnt in ((0, 4), (3, 1), (4, 0)):                           # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.census_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL and g.census_count() == (3, 0)
    fn, out, got = g.lib.f["census_read"], np.zeros(2 * 5 * 16, np.uint64), _ffi.C.c_uint32(77)
    assert fn(g.h, 0, 3, out.ctypes.data, out.size, _ffi.C.byref(got)) == _ffi.EINVAL         # a buffer one sample short
    assert fn(g.h, 0, 2, None, out.size, _ffi.C.byref(got)) == _ffi.EINVAL and fn(g.h, 0, 2, out.ctypes.data, out.size, None) == _ffi.EINVAL
    assert got.value == 77 and not out.any()
    # census_now with a buffer that is too small: cap is respected, the header still counts every subject
    now = g.lib.f["census_now"]
    hdr, rec, cnt = np.zeros(1, _ffi.CENSUS_HEADER_DTYPE), np.zeros(3, _ffi.CENSUS_SUBJECT_DTYPE), _ffi.C.c_uint32(77)
    assert now(g.h, hdr.ctypes.data, rec.ctypes.data, 1, _ffi.C.byref(cnt)) == 0
    assert cnt.value == 1 and int(hdr[0]["subjects"]) == 2 and int(hdr[0]["stored"]) == 1
    assert words(rec[:1]).tolist() == words(before[1][-1][:1]).tolist() and not words(rec[1:]).any()
    assert now(g.h, None, rec.ctypes.data, 1, _ffi.C.byref(cnt)) == _ffi.EINVAL and now(g.h, hdr.ctypes.data, None, 1, _ffi.C.byref(cnt)) == _ffi.EINVAL
    assert now(g.h, hdr.ctypes.data, rec.ctypes.data, 1, None) == _ffi.EINVAL
    assert now(g.h, hdr.ctypes.data, None, 0, _ffi.C.byref(cnt)) == 0 and cnt.value == 0 and int(hdr[0]["subjects"]) == 2
    after = g.census_read()
    assert g.census_count() == (3, 0) and words(after[0]).tolist() == words(before[0]).tolist() and words(after[1]).tolist() == words(before[1]).tolist()
    g.close()
    t = serf_amd.create(256, fanout=3)                                   # inside a tick
    t.census_start(0, 1, 8, 4)
    t.step(2)
    t.step_begin()
    for call in (lambda: t.census_start(0, 1, 8, 4), t.census_count, lambda: t.census_read(0, 1), t.census_stop, t.census_now):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                                   # a handle destroyed with a census running
    g.census_start(0, 1, 4, 300)
    g.step(6)
    assert g.census_count() == (4, 2) and g.census_read()[0]["tick"].tolist() == [1, 2, 3, 4]
    g.close()
