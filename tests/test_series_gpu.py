"""Device-resident time series (include/serf_sim_series.h) on the GPU: each of the 64 words of every sample equals what the
reference model (tests/series_model.py) computes from the dumps of the CPU oracle stepped one tick at a time.  The HIP
handle is driven in one sim_step per stretch between two injections and read once at the end; comparisons are exact."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_track_gpu as tt
from tests.series_model import WORDS, SeriesModel, as_records
from tests.test_series import HOT_TICK, check_nontrivial, drive, scenario, variant_kw
from tests.track_model import TrackModel

pytestmark = pytest.mark.gpu


def assert_same(got, want, what):
    """got: the array series_read returned; want: the model's [samples][64] words."""
    assert got.dtype == _ffi.SERIES_DTYPE
    g = np.ascontiguousarray(got).view(np.uint64).reshape(-1, WORDS)
    assert g.shape == want.shape, f"{what}: {g.shape[0]} samples, the model has {want.shape[0]}"
    bad = np.argwhere(g != want)
    names = as_records(want[:1]).dtype.names
    msg = [f"sample {i} (tick word {int(want[i, 0])}) word {j}: HIP {int(g[i, j])} != model {int(want[i, j])}" for i, j in bad[:12].tolist()]
    assert not len(bad), f"{what}: {len(bad)} words differ of fields {names}\n" + "\n".join(msg)


def both_sides(oracle, n, s, ticks, kw, first=0, period=1, capacity=None):
    capacity = capacity or ticks
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = SeriesModel(o)
    m.start(first, period, capacity)
    drive(o, s, ticks, m.step)
    g = serf_amd.create(n, **kw)
    g.series_start(first, period, capacity)
    drive(g, s, ticks, g.step)
    return o, m, g


@pytest.mark.parametrize("variant", ["krandomnodes", "bijection", "pkt_records_16", "vshards_4", "hot_spots_krandomnodes",
                                     "hot_spots_bijection_pkt_records_16"])
def test_parity_4096_nodes_every_tick(oracle, hiplib, variant):
    n, ticks = 4096, 200
    hot = variant.startswith("hot_spots_")
    s = scenario(n, hot)
    o, m, g = both_sides(oracle, n, s, ticks, variant_kw(variant))
    assert g.series_count() == m.count() == (ticks, 0)
    got = g.series_read()          # read once, at the end
    want = m.read()
    assert_same(got, want, variant)
    assert got["tick"].tolist() == list(range(1, ticks + 1))
    check_nontrivial(o, as_records(want), int(o.dump(_ffi.ARR_ROWS)["n_failed"].astype(np.int64).sum()), hot)
    if hot:
        assert got["depth_bins"][HOT_TICK].min() > 0          # all eight bins, on the GPU, in one sample
    assert g.digest() == o.digest(), "sampling must not perturb the run"
    # parts of the buffer
    assert_same(g.series_read(10, 5), want[10:15], variant + " [10, 15)")
    assert len(g.series_read(ticks, 0)) == 0


def test_period_first_tick_capacity_and_restart(oracle, hiplib):
    """Period 7 from a first tick in the future, a buffer three short of what the run would fill; a second series after
    sim_series_stop begins at sample 0."""
    n, ticks, first, period = 4096, 200, 13, 7
    due = len(range(first, ticks, period))
    s = scenario(n)
    kw = variant_kw("krandomnodes")
    o, m, g = both_sides(oracle, n, s, ticks, kw, first, period, due - 3)
    assert g.series_count() == m.count() == (due - 3, 3)
    got = g.series_read()
    assert_same(got, m.read(), "period 7")
    assert got["tick"].tolist() == [t + 1 for t in range(first, ticks, period)][:due - 3]
    with pytest.raises(_ffi.SimError) as ei:
        g.series_start(0, 1, 8)              # one series at a time
    assert ei.value.code == _ffi.ESTATE and g.series_count() == (due - 3, 3)
    g.series_stop()
    m.stop()
    assert g.series_count() == (0, 0)
    with pytest.raises(_ffi.SimError) as ei:
        g.series_read(0, 0)
    assert ei.value.code == _ffi.ESTATE
    g.series_start(5, 2, 4)                  # a first tick that has passed: now (tick 200)
    m.start(5, 2, 4)
    g.step(9)
    m.step(9)
    assert g.series_count() == m.count() == (4, 1)
    got = g.series_read()
    assert_same(got, m.read(), "second series")
    assert got["tick"].tolist() == [201, 203, 205, 207]
    assert g.digest() == o.digest()


def test_series_and_trackers_on_one_handle(oracle, hiplib):
    """tests/test_track_gpu.py's trackers and a series of period 3 together: each equals its own model, which does not know
    the other."""
    n, ticks = 4096, 160
    kw = dict(tt.KW, flags=tt.KRANDOM)
    s = tt.script(n)
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    tm = TrackModel(o)
    sm = SeriesModel(o, tm.evaluate)
    sm.start(0, 3, 1000)
    mh = tt.drive(o, s, ticks, lambda specs: [tm.add(x) for x in specs], sm.step)
    want_trk = [tm.result(h) for h in mh]
    g = serf_amd.create(n, **kw)
    g.series_start(0, 3, 1000)
    ids = tt.drive(g, s, ticks, g.track_add, g.step)
    tt.assert_same([r.as_dict() for r in g.track_read(ids)], want_trk, "trackers next to a series")
    assert any(r["p99"] != _ffi.TRACK_NEVER for r in want_trk)
    assert g.series_count() == sm.count() == (len(range(0, ticks, 3)), 0)
    assert_same(g.series_read(), sm.read(), "a series next to trackers")
    assert g.digest() == o.digest()


def test_parity_at_size_65536_nodes(oracle, hiplib):
    n, ticks = 65536, 200
    kw = dict(tt.KW, view_slots=16, flags=tt.KRANDOM)
    s = scenario(n)
    o, m, g = both_sides(oracle, n, s, ticks, kw, 0, 5, 1000)
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    assert g.series_count() == m.count() == (40, 0)
    got = g.series_read()
    assert_same(got, m.read(), "65536 nodes")
    assert got["timers"].max() > 0 and got["records"][:, _ffi.K_EVENT - 1].max() > 0 and got["running"].min() == n - 6
    assert g.digest() == o.digest()


def test_errors_leave_everything_as_it_was(hiplib):
    n = 4096
    kw = variant_kw("krandomnodes")
    sh = serf_amd.create(n, force_sharded=True, **kw)      # a shard has no series
    for call in (lambda: sh.series_start(0, 1, 8), sh.series_count, lambda: sh.series_read(0, 0), sh.series_stop):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    g = serf_amd.create(n, **kw)
    assert g.series_count() == (0, 0)
    for call in (lambda: g.series_read(0, 0), g.series_stop):           # no series yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    for args in ((0, 0, 8), (0, 1, 0), (0, 1, _ffi.SERIES_MAX_SAMPLES + 1)):
        with pytest.raises(_ffi.SimError) as ei:
            g.series_start(*args)
        assert ei.value.code == _ffi.EINVAL and g.series_count() == (0, 0)
    g.series_start(0, 1, 8)
    g.step(3)
    assert g.series_count() == (3, 0)
    for first, cnt in ((0, 4), (3, 1), (4, 0)):                          # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.series_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL and g.series_count() == (3, 0)
    g.close()
    t = serf_amd.create(256, fanout=3)                                   # inside a tick
    t.series_start(0, 1, 8)
    t.step(2)
    t.step_begin()
    for call in (lambda: t.series_start(0, 1, 8), t.series_count, lambda: t.series_read(0, 1), t.series_stop):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                                   # a handle destroyed with a series running
    g.series_start(0, 1, 4)
    g.step(6)
    assert g.series_count() == (4, 2) and g.series_read()["tick"].tolist() == [1, 2, 3, 4]
    g.close()
