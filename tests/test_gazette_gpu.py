"""The member gazette of the HIP library (include/serf_sim_gazette.h) against the reference model (tests/gazette_model.py) on the
oracle stepped one tick at a time: the scenarios of tests/test_gazette.py.  The HIP handle advances in long sim_step calls and is
read once at the end; every operation is injected up front.  Every sample word, both whole maps and the rankings are compared
exactly, and the digest equals the oracle's in every test."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_gazette as tg
from tests import test_ledger as tl
from tests import test_observer_shapes as shapes
from tests.gazette_model import GazetteModel

pytestmark = pytest.mark.gpu
W = _ffi.GAZETTE_WORDS
KS = (1, 10, 64)


def words(a):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(a))).view(np.uint64).reshape(-1)


def same_words(got, want, what, per=W):
    g, w = words(got).reshape(-1, per), words(want).reshape(-1, per)
    assert g.shape == w.shape, f"{what}: {g.shape[0]} records, the model has {w.shape[0]}"
    bad = np.argwhere(g != w)
    assert not len(bad), f"{what}: word {bad[0][1]} of record {bad[0][0]}: HIP {g[tuple(bad[0])]} != model {w[tuple(bad[0])]}"


def same_map(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: row {bad[0][0]} column {bad[0][1]}: HIP {got[tuple(bad[0])]} != model {want[tuple(bad[0])]}; {len(bad)} differ"


def same_tops(g, m, what, ks=KS):
    for which in (_ffi.GAZETTE_MAP_NODES, _ffi.GAZETTE_MAP_SUBJECTS):
        for col in range(_ffi.GAZETTE_COLS):
            for k in ks:
                got, want = g.gazette_top(which, col, k), m.top(which, col, k)
                assert got["id"].tolist() == want["id"].tolist(), f"{what}: map {which} column {col} k {k}"
                assert (got["row"] == want["row"]).all(), f"{what}: map {which} column {col} k {k}: rows"


def same_gazette(g, m, o, what, tops=False):
    """Everything a running gazette on handle g says against the model m behind the oracle o."""
    assert g.gazette_count() == m.count(), what
    same_words(g.gazette_read(), m.read(), what + ": samples")
    same_map(g.gazette_nodes(), m.nodes, what + ": node map")
    same_map(g.gazette_subjects(), m.subj, what + ": subject map")
    n = m.n
    if n > 5:
        same_map(g.gazette_nodes(3, 2), m.nodes[3:5], what + ": a slice of the node map")
        same_map(g.gazette_subjects(n - 2, 2), m.subj[n - 2:], what + ": the subject map's last rows")
    if tops:
        same_tops(g, m, what)
    assert g.digest() == o.digest(), what


def hip_run(name, arg=None):
    n, kw, drive, start = tg.scenario(name, arg)
    g = serf_amd.create(n, **kw)
    g.gazette_start(**start)
    drive(g, g.step)
    return g


def same_run(name, arg=None, tops=False):
    r = tg.run(name, arg)
    g = hip_run(name, arg)
    same_gazette(g, r["m"], r["o"], f"{name} {arg}", tops)
    return g, r


# ---- 1. the scenario ----
@pytest.mark.parametrize("period", (1, 3))
@pytest.mark.parametrize("fan", sorted(shapes.FANOUTS))
def test_the_scenario(hiplib, fan, period):
    """1 000 nodes: crashes, leaves, a Reaper that reaps, a force-leave with prune, a revive inside flap_window and one outside."""
    g, r = same_run("main", (fan, period), tops=period == 1)
    tot = r["samples"]["sums"].astype(np.int64).sum(axis=0)
    assert (tot[:6] > 0).all()
    g.close()


def test_flap_window_is_exclusive(hiplib):
    """flap_window set to a dead time that the scenario's joins out of Failed really have, and to one tick more."""
    w = tg.edge_window()
    for window in (w, w + 1):
        g, r = same_run("main", ("krandomnodes", 1, window))
        g.close()


# ---- 2. cluster sizes ----
@pytest.mark.parametrize("n", (3, 64, 65, 257))
def test_cluster_sizes(hiplib, n):
    """Less than a wave; one wave with a dense view (view_slots == n_nodes); a ragged wave; two workgroups."""
    g, r = same_run("ragged", n, tops=True)
    assert r["samples"]["sums"].astype(np.int64).sum() > 0
    if n == 64:
        assert r["samples"]["slots"].max() == 64, "a dense view: every node is a subject"
    g.close()


def test_four_virtual_shards_on_one_handle(hiplib):
    g, r = same_run("vshards")
    assert r["samples"]["sums"].astype(np.int64).sum() > 0
    g.close()


def test_second_pass(hiplib):
    """GAZETTE_GRID x BLOCK + 65 nodes: the scan's pass loop takes a second turn, of one whole wave and one lane, and adds to
    the partial counts of the first.  The crashed node n - 1 and its first accusers lie in either pass."""
    g, r = same_run("second")
    s = r["samples"]
    assert s["tick"].tolist() == [1, 6, 11, 16] and s["running"][-1] == tg.second_n() - 2
    assert s["sums"].astype(np.int64)[:, 5].sum() > 0, "nobody suspected anybody: the second pass shows nothing"
    assert (r["nodes"][tg.gazette_grid() * tg.BLOCK:, 5] > 0).any() or (r["subjects"][tg.second_n() - 1, 5] > 0)
    g.close()


def test_nobody_runs(hiplib):
    """Every node crashes: the sums stay 0 while the shadow still moves."""
    g, r = same_run("idle")
    assert r["samples"]["running"][-1] == 0
    g.close()


# ---- 3. fresh slots ----
@pytest.mark.parametrize("period", (1, 5))
def test_recycled_slots_go_to_other_subjects(hiplib, period):
    g, r = same_run("recycle", period)
    assert r["m"].rehomed >= 2 and r["samples"]["fresh"].sum() > r["m"].rehomed
    g.close()


def test_the_high_water_mark_crosses_shadow_groups(hiplib):
    """200 view slots: a group of the shadow holds four slots; the run starts with none and ends with eight."""
    g, r = same_run("groups")
    assert r["samples"]["slots"][0] == 0 and r["samples"]["slots"][-1] == 8
    g.close()


# ---- 4. starts, stops, a full buffer ----
def pair(n, kw):
    o = tl.maker(n, kw)()
    return o, GazetteModel(o), serf_amd.create(n, **kw)


def test_started_late_stopped_and_started_again(hiplib):
    n, kw, _, _ = tg.scenario("groups")
    o, m, g = pair(n, kw)
    for s in (o, g):
        tg.main_drive(0)(s, lambda k: None)                      # the operations, no tick yet
    m.step(30), g.step(30)
    m.start(10, 2, 100, 40), g.gazette_start(10, 2, 100, 40)     # a first tick that has passed: now
    m.step(25), g.step(25)
    assert g.gazette_count() == (13, 0) and m.read()["tick"][0] == 31
    same_gazette(g, m, o, "started late")
    m.stop(), g.gazette_stop()
    assert g.gazette_count() == (0, 0)
    m.step(5), g.step(5)
    m.start(o.tick + 3, 1, 100, 40), g.gazette_start(g.tick + 3, 1, 100, 40)
    m.step(40), g.step(40)
    assert g.gazette_count() == (37, 0)
    same_gazette(g, m, o, "started again", tops=True)
    assert m.read()["sums"].astype(np.int64).sum() > 0
    g.close()


def test_a_full_buffer_stops_the_maps(hiplib):
    """Samples that are due with the buffer full are dropped and counted; the shadow and the maps stand where the last stored
    sample left them: the maps are the sums of the samples that can be read."""
    n, kw, _, _ = tg.scenario("groups")
    o, m, g = pair(n, kw)
    m.start(0, 1, 20, 60), g.gazette_start(0, 1, 20, 60)
    tg.main_drive(100)(o, m.step)
    tg.main_drive(100)(g, g.step)
    assert g.gazette_count() == (20, 80)
    same_gazette(g, m, o, "full buffer")
    assert g.gazette_nodes()[:, :7].astype(np.int64).sum(axis=0).tolist() == g.gazette_read()["sums"].astype(np.int64).sum(axis=0).tolist()
    g.close()


# ---- 5. beside the other observers ----
def test_beside_all_eleven_other_observers(hiplib):
    """Every observer the library has on one handle: the gazette's words are the model's, and the digest is a plain run's."""
    n, kw, drive, start = tg.scenario("groups")
    r = tg.run("groups")
    plain = serf_amd.create(n, **kw)
    drive(plain, plain.step)
    g = serf_amd.create(n, **kw)
    ticks, entries = 100, [(_ffi.K_JOIN, 3, 1)]
    g.series_start(0, 1, ticks), g.census_start(0, 1, ticks, 8), g.roll_start(0, 1, ticks), g.ledger_start(entries, 0, 1, ticks)
    g.detect_start(0, 1, ticks), g.spread_start(entries, 0, 1, ticks), g.traffic_start(0, 1, ticks), g.tree_start(entries, 0, ticks)
    g.qboard_start([777], 0, 1, ticks), g.catalog_start()
    ids = g.track_add([_ffi.rumour_tracker(*entries[0])])
    g.gazette_start(**start)
    drive(g, g.step)
    same_gazette(g, r["m"], r["o"], "beside the others", tops=True)
    assert g.digest() == plain.digest() == r["o"].digest()
    for count in (g.series_count, g.census_count, g.roll_count, g.ledger_count, g.detect_count, g.spread_count, g.traffic_count,
                  g.tree_count, g.qboard_count):
        assert count() == (ticks, 0)
    assert g.catalog_count()[0] == ticks and len(g.track_read(ids)) == 1
    g.close(), plain.close()


# ---- 6. checkpoints ----
def test_started_on_a_restored_handle(hiplib):
    n, kw, _, start = tg.scenario("main", ("krandomnodes", 1))
    src = tl.maker(n, kw)()
    tg.main_drive(90)(src, src.step)
    image = src.snapshot()
    o, m, g = pair(n, kw)
    o.restore(image), g.restore(image)
    m.restored()
    m.start(**start), g.gazette_start(**start)
    m.step(40), g.step(40)
    s = m.read()
    assert s["tick"][0] == 91 and s["slots"][0] >= 6 and s["fresh"][0] == 0 and s["sums"].astype(np.int64).sum() > 0
    same_gazette(g, m, o, "started on a restored handle")
    g.close()


@pytest.mark.parametrize("period", (1, 3))
def test_an_image_restored_under_a_running_gazette(hiplib, period):
    """The gazette is started on the fresh handle, sim_restore (which takes a fresh handle) leaves it running; the first sample
    behind the restore does not follow the start's shadow by one period: it re-takes the whole shadow and counts nothing."""
    n, kw, _, start = tg.scenario("main", ("krandomnodes", period))
    src = tl.maker(n, kw)()
    tg.main_drive(90)(src, src.step)
    image = src.snapshot()
    o, m, g = pair(n, kw)
    m.start(**start), g.gazette_start(**start)
    o.restore(image), g.restore(image)
    m.restored()
    m.step(42), g.step(42)
    s = m.read()
    assert len(s) == 42 // period and s["tick"][0] == 91
    assert s["fresh"][0] == s["slots"][0] >= 6 and not s["sums"][0].any() and not s["matrix"][0].any() and not s["swim"][0].any()
    assert not s["fresh"][1:].any() and s["sums"][1:].astype(np.int64).sum() > 0, "nothing happens behind the restore"
    same_gazette(g, m, o, "restored under a running gazette")
    g.close()


# ---- 7. the rankings' ties ----
def test_all_keys_tied_right_behind_the_start(hiplib):
    g = serf_amd.create(300, **shapes.ragged_kw(300, "krandomnodes"))
    g.gazette_start()
    for which in (0, 1):
        for col in range(8):
            for k in KS:
                top = g.gazette_top(which, col, k)
                assert top["id"].tolist() == list(range(k)) and not top["row"].any()
    g.close()
    g = serf_amd.create(3, **shapes.ragged_kw(3, "krandomnodes"))      # fewer rows than places
    g.gazette_start()
    top = g.gazette_top(1, 2, 10)
    assert top["id"].tolist() == [0, 1, 2] + [0xFFFFFFFF] * 7 and not top["row"].any()
    g.close()


def test_a_tie_across_a_workgroup_boundary(hiplib):
    """257 nodes; 255 and 256 crash in one tick: every running node announces both Failed — rows 255 (the last of the first
    workgroup) and 256 (the only one of the second) of the subject map tie in `failed`, and the two lead the ranking in
    ascending id."""
    r = tg.run("boundary")
    g = hip_run("boundary")
    same_gazette(g, r["m"], r["o"], "boundary", tops=True)
    top = g.gazette_top(_ffi.GAZETTE_MAP_SUBJECTS, _ffi.GAZETTE_FAILED, 10)
    assert top["id"][:3].tolist() == [255, 256, 0] and top["row"][0][2] == top["row"][1][2] == 255
    g.close()


# ---- 8. errors ----
def test_errors_leave_everything_as_it_was(hiplib):
    n, kw = 257, shapes.ragged_kw(257, "krandomnodes")
    every = lambda s: (s.gazette_start, s.gazette_count, lambda: s.gazette_read(0, 0), lambda: s.gazette_nodes(0, 1),
                       lambda: s.gazette_subjects(0, 1), lambda: s.gazette_top(0, 0, 1), s.gazette_stop)
    sh = serf_amd.create(4096, force_sharded=True, **tl.census_kw("krandomnodes"))          # a shard has no gazette
    for call in every(sh):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    g = serf_amd.create(n, **kw)
    assert g.gazette_count() == (0, 0)
    for call in every(g)[2:]:                                              # no gazette yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    for args in ((0, 0, 8, 60), (0, 1, 0, 60), (0, 1, _ffi.GAZETTE_MAX_SAMPLES + 1, 60), (0, 1, 8, 1 << 21), (0, 1, 8, 0xFFFFFFFF)):
        with pytest.raises(_ffi.SimError) as ei:
            g.gazette_start(*args)
        assert ei.value.code == _ffi.EINVAL and g.gazette_count() == (0, 0), args
    g.inject(2, _ffi.OP_CRASH, 7)
    g.gazette_start(0, 1, 64, (1 << 21) - 1)
    with pytest.raises(_ffi.SimError) as ei:
        g.gazette_start()                                                  # a double start
    assert ei.value.code == _ffi.ESTATE
    g.step(30)
    before = (g.gazette_read(), g.gazette_nodes(), g.gazette_subjects())
    assert before[0]["sums"].astype(np.int64)[:, 5].sum() > 0
    bad = [lambda: g.gazette_read(0, 31), lambda: g.gazette_read(30, 1), lambda: g.gazette_nodes(0, n + 1), lambda: g.gazette_nodes(n, 1),
           lambda: g.gazette_subjects(n - 1, 2), lambda: g.gazette_top(2, 0, 1), lambda: g.gazette_top(0, 8, 1),
           lambda: g.gazette_top(0, 0, 0), lambda: g.gazette_top(0, 0, 65)]
    for call in bad:
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.EINVAL
    f, C = g.lib.f, _ffi.C
    got = C.c_uint32(77)
    small = np.zeros(2 * W, np.uint64)
    assert f["gazette_read"](g.h, 0, 3, small.ctypes.data, small.size, C.byref(got)) == _ffi.EINVAL          # a buffer one sample short
    assert f["gazette_read"](g.h, 0, 2, None, small.size, C.byref(got)) == _ffi.EINVAL
    assert f["gazette_nodes"](g.h, 0, 1, None) == _ffi.EINVAL and f["gazette_top"](g.h, 0, 0, 1, None) == _ffi.EINVAL
    assert f["gazette_start"](None, 0, 1, 8, 60) == _ffi.EINVAL and f["gazette_count"](g.h, None, C.byref(got)) == _ffi.EINVAL
    assert got.value == 77 and not small.any()
    assert len(g.gazette_nodes(n, 0)) == 0                                 # an empty slice at the end is no read beyond it
    after = (g.gazette_read(), g.gazette_nodes(), g.gazette_subjects())
    same_words(after[0], before[0], "behind the refused calls")
    same_map(after[1], before[1], "behind the refused calls"), same_map(after[2], before[2], "behind the refused calls")
    g.step_begin()                                                         # inside a tick
    for call in every(g):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    g.close()                                                              # (destroyed inside a tick, with a gazette running)
    g = serf_amd.create(256, fanout=3)                                     # a handle destroyed with a gazette running and a full buffer
    g.gazette_start(0, 1, 4)
    g.step(6)
    assert g.gazette_count() == (4, 2) and g.gazette_read()["tick"].tolist() == [1, 2, 3, 4]
    g.close()
