"""The detection log of the HIP library through the scenarios of tests/test_detect_shapes.py — ragged ranges, two closes per slot
in every wave and three chunks, a pair across the end of the log, a cluster in which nobody runs, observers started on a restored
handle, all seven observers on one handle: every header word, every log record and every open episode equal to the reference
model's (tests/detect_model.py on the CPU oracle), and the digest equal to the oracle's.  Which scenario is there for which line
of detect_kernel: that file's docstring and profiles/detect_shapes.md.  The HIP handle advances in one or two long sim_step calls
and is read once at the end; comparisons are exact."""
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_detect_shapes as ds
from tests import test_observer_resume as rs
from tests import test_observer_shapes as sh
from tests.test_census_gpu import assert_same as census_same
from tests.test_detect_gpu import assert_same, same_words
from tests.test_ledger_gpu import assert_same as ledger_same
from tests.test_observer_resume_gpu import resumed, two_calls
from tests.test_roll_gpu import assert_same as roll_same
from tests.test_series_gpu import assert_same as series_same
from tests.test_spread_gpu import same_reads as spread_reads, same_samples as spread_samples
from tests.test_track_gpu import assert_same as track_same
from tests.test_traffic_gpu import same_reads as traffic_reads

pytestmark = pytest.mark.gpu


def hip_run(n, kw, script, ticks, run, what, log_capacity=ds.LOG_CAPACITY):
    """script(sim, step) on the HIP library with a log behind every tick, read once at the end, against the cached oracle run."""
    g = serf_amd.create(n, **kw)
    g.detect_start(0, 1, ticks, log_capacity)
    script(g, g.step)
    assert g.tick == ticks and g.detect_count() == run["m"].count(), what
    assert_same(g, run["want"], what)                      # (first: a failure names the first word that differs)
    assert g.detect_log_count() == run["m"].log_count(), what
    assert g.digest() == run["o"].digest(), what + ": a detection log must not perturb the run"
    return g


# ---- 1. ragged ranges ----
@pytest.mark.parametrize("n,fan", ds.RAGGED_CASES)
def test_ragged(hiplib, n, fan):
    """ragged(n), dense: n slots in two calls of sim_step (10 and 80 ticks).  The slots that close are the last two of the range."""
    run = ds.ragged_oracle(n, fan)
    ds.check_ragged(n, run)
    hip_run(n, ds.ragged_kw(n, fan), ds.ragged_drive(n), ds.RAGGED_TICKS, run, f"ragged({n}) {fan}").close()


# ---- 2. two closes per slot ----
def test_two_closes_per_slot_in_every_wave_and_three_chunks(hiplib):
    """600 slots, one call of sim_step: the sample with tick word 131 closes 28 episodes, two in each of 14 slots that lie in all
    four waves of the first chunk and in three chunks."""
    run = ds.double_oracle()
    ds.check_double(run)
    g = hip_run(ds.DOUBLE_N, ds.DOUBLE_KW, ds.double_drive(ds.DOUBLE_VICTIMS, ds.DOUBLE_TICKS), ds.DOUBLE_TICKS, run, "two closes per slot")
    ds.check_pairs(g.detect_log(), list(ds.DOUBLE_VICTIMS), 14)
    g.close()


# ---- 3. a pair across the end of the log ----
@pytest.mark.parametrize("cap", ds.STRADDLE_CAPS)
def test_a_pair_across_the_end_of_the_log(hiplib, cap):
    """log_capacity 15: the last record is slot 64's STOPPED and its DETECTED is lost; 14: the end falls between two slots; 16:
    slot 64's DETECTED is the last record that fits."""
    run, full = ds.straddle_oracle(cap), ds.straddle_oracle(ds.LOG_CAPACITY)
    ds.check_straddle(cap, run, full)
    script = ds.double_drive(ds.STRADDLE_VICTIMS, ds.STRADDLE_TICKS, (ds.STRADDLE_LATE,))
    g = hip_run(ds.STRADDLE_N, ds.DOUBLE_KW, script, ds.STRADDLE_TICKS, run, f"log_capacity {cap}", log_capacity=cap)
    assert g.detect_log_count() == (cap, ds.STRADDLE_RECORDS - cap)
    same_words(g.detect_log(), full["want"][1][:cap], _ffi.DETECT_EPISODE_WORDS, f"log_capacity {cap}: the prefix of the full log", str)
    with pytest.raises(_ffi.SimError) as ei:
        g.detect_log(cap, 1)                               # beyond what was written
    assert ei.value.code == _ffi.EINVAL
    assert len(g.detect_log(cap, 0)) == 0
    g.close()


# ---- 4. nobody runs ----
@pytest.mark.parametrize("n,fan", ds.IDLE_CASES)
def test_nobody_runs(hiplib, n, fan):
    """Every node crashes at tick 5: seven samples with R == 0, in which no DOWN episode latches half, p99 or all."""
    run = ds.idle_oracle(n, fan)
    ds.check_idle(n, run)
    g = hip_run(n, ds.idle_kw(fan), ds.idle_drive(n), sh.IDLE_TICKS, run, f"nobody_runs({n}) {fan}")
    assert g.detect_log_count() == (0, 0) and len(g.detect_open()) == n
    g.close()


# ---- 5. observers started on a restored handle ----
@pytest.mark.parametrize("fan", sorted(sh.FANOUTS))
def test_a_log_started_on_a_restored_handle(hiplib, fan):
    """sim_restore to tick 10 of ragged(65), then sim_detect_start: `first` holds for the sample behind tick 10, where node 64 is
    down already — CENSORED.  Two calls of sim_step (7, then the rest)."""
    run = ds.resumed_detect_oracle(fan)
    ds.check_resumed_detect(fan, run)
    case, img, cond, ref = rs.ragged_run(ds.RESUMED_N, fan)
    what = f"a log started on a restored handle, {fan}"
    g = resumed(case, img)
    g.detect_start(0, 1, case.ticks, ds.LOG_CAPACITY)
    assert g.detect_count() == (0, 0)
    case.after(g, two_calls(g), ref["setup"])
    assert g.tick == case.ticks and g.detect_count() == run["m"].count()
    assert_same(g, run["want"], what)
    assert g.detect_log_count() == run["m"].log_count()
    assert g.digest() == run["o"].digest(), what
    g.close()


def test_a_spread_map_started_on_a_restored_handle(hiplib):
    fan = "krandomnodes"
    run = ds.resumed_spread_oracle(fan)
    ds.check_resumed_spread(run, fan)
    case, img, cond, ref = rs.ragged_run(ds.RESUMED_N, fan)
    what = "a spread map started on a restored handle"
    g = resumed(case, img)
    g.spread_start(run["entries"], 0, 1, case.ticks)
    case.after(g, two_calls(g), ref["setup"])
    assert g.tick == case.ticks and g.spread_count() == run["m"].count()
    spread_samples(g.spread_read(), run["samples"], what)
    spread_reads(g, run["m"], what, top_ks=(7,))
    assert g.digest() == run["o"].digest(), what
    g.close()


def test_a_traffic_meter_started_on_a_restored_handle(hiplib):
    fan = "bijection"
    run = ds.resumed_traffic_oracle(fan)
    ds.check_resumed_traffic(run, fan)
    case, img, cond, ref = rs.ragged_run(ds.RESUMED_N, fan)
    what = "a traffic meter started on a restored handle"
    g = resumed(case, img)
    g.traffic_start(0, 1, case.ticks)
    case.after(g, two_calls(g), ref["setup"])
    assert g.tick == case.ticks
    traffic_reads(g, run["m"], what, top_ks=(1, 10))
    assert g.digest() == run["o"].digest(), what
    g.close()


# ---- 6. all seven observers and two trackers on one handle ----
def test_all_seven_observers_and_two_trackers_on_one_handle(hiplib):
    """The cluster and the script of test_ledger_gpu.test_all_five_observers_on_one_handle with the detection log, the spread map
    and the traffic meter next to the four older samplers, periods 1, 2, 3, 1, 1, 2, 3, one sim_step per stretch: each equals its
    own model, which does not know the others."""
    run = ds.seven_oracle()
    ds.check_seven(run)
    ms = run["models"]
    g = serf_amd.create(ds.SEVEN_N, **ds.SEVEN_KW)
    ds.seven_start(dict(series=g.series_start, census=g.census_start, roll=g.roll_start, ledger=g.ledger_start, detect=g.detect_start,
                        spread=g.spread_start, traffic=g.traffic_start))
    ids, events = ds.seven_script(g, lambda spec: g.track_add([spec])[0], g.step)
    assert events == run["events"]
    track_same([r.as_dict() for r in g.track_read(ids)], run["trackers"], "two trackers next to the seven")
    counts = dict(series=g.series_count(), census=g.census_count(), roll=g.roll_count(), ledger=g.ledger_count(), detect=g.detect_count(),
                  spread=g.spread_count(), traffic=g.traffic_count())
    assert counts == {k: m.count() for k, m in ms.items()}
    series_same(g.series_read(), ms["series"].read(), "a series next to the others")
    census_same(g.census_read(), ms["census"].read(), "a census next to the others")
    roll_same(g.roll_read(), ms["roll"].read(), "a roll next to the others")
    ledger_same(g.ledger_read(), ms["ledger"].read(), "a ledger next to the others")
    assert g.detect_log_count() == ms["detect"].log_count()
    assert_same(g, ds.model_of(ms["detect"]), "a detection log next to the others")
    spread_samples(g.spread_read(), ms["spread"].read(), "a spread map next to the others")
    spread_reads(g, ms["spread"], "a spread map next to the others", top_ks=(7,))
    traffic_reads(g, ms["traffic"], "a traffic meter next to the others")
    assert g.digest() == run["o"].digest()
    g.close()
