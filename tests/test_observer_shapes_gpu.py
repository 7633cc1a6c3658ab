"""The observers of the HIP library at the cluster sizes of tests/test_observer_shapes.py — ragged, tiny, idle, and beyond what one
pass of a kernel's grid covers: the same scripts as on the oracle, every word of every tracker, series sample and census sample
and every answer read at the end equal to the reference models' (which size is there for which wrong guard: that file's
docstring).  The HIP handle advances in long sim_step calls and is read once at the end; comparisons are exact."""
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_observer_shapes as sh
from tests.test_census_gpu import assert_same as census_same
from tests.test_series_gpu import assert_same as series_same
from tests.test_track_gpu import assert_same as track_same

pytestmark = pytest.mark.gpu


def one(g):
    return lambda spec: g.track_add([spec])[0]


def read_trackers(g, hs):
    names = sorted(hs)
    return names, [r.as_dict() for r in g.track_read([hs[k] for k in names])]


def same_answers(got, want, what):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], f"{what}: {k}: HIP {got[k]} != oracle {want[k]}"


@pytest.mark.parametrize("fan", sorted(sh.FANOUTS))
@pytest.mark.parametrize("n", sh.RAGGED_SIZES)
def test_ragged(hiplib, n, fan):
    """ragged(n) with all three observers on one handle, in two calls of sim_step (10 and 80 ticks), everything read once at the end."""
    want = sh.ragged_oracle(n, fan)
    sh.check_ragged(n, want)
    what = f"ragged({n}) {fan}"
    g = serf_amd.create(n, **sh.ragged_kw(n, fan))
    g.series_start(0, 1, sh.RAGGED_TICKS)
    g.census_start(0, 1, sh.RAGGED_TICKS, sh.CENSUS_SUBJECTS)
    hs, ru = sh.ragged_script(g, n, one(g), g.step)
    assert ru == want["rumours"] and sorted(hs) == sorted(want["trackers"])
    names, got = read_trackers(g, hs)
    track_same(got, [want["trackers"][k] for k in names], f"{what} {names}")
    assert g.series_count() == (sh.RAGGED_TICKS, 0) and g.census_count() == (sh.RAGGED_TICKS, 0)
    series_same(g.series_read(), want["series"], what)
    census_same(g.census_read(), want["census"], what)
    same_answers(sh.answers(g, n, ru, want["noslot"]), want["answers"], what)
    g.close()


@pytest.mark.parametrize("fan", sorted(sh.FANOUTS))
@pytest.mark.parametrize("n", sh.IDLE_SIZES)
def test_nobody_runs(hiplib, n, fan):
    """Every node crashes at tick 5: seven samples and evaluations of a cluster in which no node runs."""
    want = sh.idle_oracle(n, fan)
    sh.check_idle(n, want)
    what = f"nobody_runs({n}) {fan}"
    g = serf_amd.create(n, **dict(sh.KW, view_slots=0, flags=sh.FANOUTS[fan]))
    g.series_start(0, 1, sh.IDLE_TICKS)
    g.census_start(0, 1, sh.IDLE_TICKS, sh.CENSUS_SUBJECTS)
    hs = sh.idle_script(g, n, one(g), g.step)
    names, got = read_trackers(g, hs)
    track_same(got, [want["trackers"][k] for k in names], f"{what} {names}")
    series_same(g.series_read(), want["series"], what)
    census_same(g.census_read(), want["census"], what)
    same_answers(sh.idle_answers(g), want["answers"], what)
    g.close()


def test_series_second_pass(hiplib):
    """SER_CAP + 65 nodes: series_sample_kernel's pass loop takes a second turn, of one whole wave and one lane."""
    o, want = sh.series_second_pass_oracle()
    sh.check_series_second_pass(want)
    n = sh.SERIES_N
    g = serf_amd.create(n, **sh.BIG_KW)
    g.series_start(0, sh.SERIES_PERIOD, 100)
    sh.big_start(g, n)
    g.step(sh.SERIES_TICKS)
    assert g.series_count() == (3, 0)
    series_same(g.series_read(), want, f"{n} nodes")
    assert g.digest() == o.digest()
    g.close()


def test_trackers_second_pass(hiplib):
    """TRK_CAP + 65 nodes: track_count_kernel's pass loop takes a second turn; an event tracker over all 14 ticks, a suspicion
    and a JOIN tracker inside a window of four."""
    o, want = sh.track_second_pass_oracle()
    sh.check_track_second_pass(want)
    n = sh.TRACK_N
    g = serf_amd.create(n, **sh.BIG_KW)
    hs = sh.track_second_pass_script(g, n, one(g), g.step)
    names, got = read_trackers(g, hs)
    track_same(got, [want[k] for k in names], f"{n} nodes {names}")
    assert g.digest() == o.digest()
    g.close()


def test_convergence_second_pass(hiplib):
    """CONV_CAP + 65 nodes: convergence_many_kernel's loop takes a second round, for sim_convergence and for 64 rumours at once."""
    o, ev, want = sh.conv_second_pass_oracle()
    sh.check_conv_second_pass(want)
    n = sh.CONV_N
    g = serf_amd.create(n, **sh.BIG_KW)
    assert sh.big_start(g, n) == ev
    g.step(sh.CONV_TICKS)
    same_answers(sh.conv_second_pass_answers(g, n, ev), want, f"{n} nodes")
    g.close()
