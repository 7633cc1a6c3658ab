"""The observers of the HIP library across a checkpoint — the cases of tests/test_observer_resume.py: observers started on a handle
that sim_restore has just rebuilt from an oracle's image, the `_now` entry points on such a handle before its first step,
observers and trackers that exist before sim_restore, and snapshots taken in the middle of an observed run.  The reference is
that file's: the models on an oracle that never restored (for the observers that exist before the restore: on an oracle that
makes the same jump).  The HIP handle advances in one or two long sim_step calls and is read once at the end; every word of
every sample, tracker result and answer is compared exactly, and the digest at the end equals the oracle's."""
import numpy as np
import pytest

import serf_amd
from tests import test_ledger as tl
from tests import test_observer_resume as rs
from tests import test_observer_shapes as sh
from tests.test_census_gpu import assert_same as census_same
from tests.test_lazy_planes_gpu import _create as create_lazy
from tests.test_ledger_gpu import assert_same as ledger_same
from tests.test_observer_shapes_gpu import same_answers
from tests.test_roll_gpu import assert_same as roll_same
from tests.test_series_gpu import assert_same as series_same
from tests.test_track_gpu import assert_same as track_same

pytestmark = pytest.mark.gpu
FIRST_CALL = 7                   # ticks of the first of the two sim_step calls behind a restore


def words(a):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(a))).view(np.uint64).reshape(-1)


def same_words(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, f"{what}: {g.shape[0]} words, the model has {w.shape[0]}"
    bad = np.nonzero(g != w)[0]
    assert not len(bad), f"{what}: {len(bad)} words differ, the first at {bad[0]}: HIP {int(g[bad[0]])} != model {int(w[bad[0]])}"


def start(g, plan):
    g.series_start(*plan["series"])
    g.census_start(*plan["census"])
    g.roll_start(*plan["roll"])
    g.ledger_start(*plan["ledger"])


def add(g, specs):
    return dict(zip([name for name, _ in specs], g.track_add([spec for _, spec in specs])))


def two_calls(g):
    def step(k):
        g.step(min(k, FIRST_CALL))
        if k > FIRST_CALL:
            g.step(k - FIRST_CALL)
    return step


def same_trackers(g, ids, want, what):
    names = sorted(ids)
    assert names == sorted(want)
    got = [r.as_dict() for r in g.track_read([ids[k] for k in names])]
    track_same(got, [want[k] for k in names], f"{what} {names}")


def same_reads(g, want, what):
    """Everything read once, at the end."""
    counts = dict(series=g.series_count(), census=g.census_count(), roll=g.roll_count(), ledger=g.ledger_count())
    assert counts == want["counts"], f"{what}: (taken, dropped): HIP {counts} != models {want['counts']}"
    series_same(g.series_read(), want["series"], what)
    census_same(g.census_read(), want["census"], what)
    roll_same(g.roll_read(), want["roll"], what)
    ledger_same(g.ledger_read(), want["ledger"], what)


def same_now(g, setup, want, what):
    """The `_now` entry points and the ABI's own answers about the state the handle is in."""
    abi, (census, roll, ledger) = want
    _, _, _, top_k, by = setup["plan"]["roll"]
    for got, model, name in zip(g.ledger_now(setup["plan"]["ledger"][0]), ledger, ("ledger_now header", "ledger_now records")):
        same_words(got, model, f"{what}: {name}")           # (first: nothing has built the graph of the packets in flight yet)
    for got, model, name in zip(g.census_now(64), census, ("census_now header", "census_now records")):
        same_words(got, model, f"{what}: {name}")
    for got, model, name in zip(g.roll_now(top_k, by, nodes=True), roll, ("roll_now header", "roll_now top", "roll_now nodes")):
        same_words(got, model, f"{what}: {name}")
    same_answers(rs.abi_answers(g, setup["asked"]), abi, what)


def resumed(case, img, g=None):
    g = g or serf_amd.create(case.n, **case.kw)
    g.restore(img)
    assert g.tick == case.T
    return g


def carry_and_compare(case, g, ref):
    """Observers started and trackers added on the restored handle at T, the rest of the script, everything read at the end."""
    setup = ref["setup"]
    start(g, setup["plan"])
    ids = add(g, setup["specs"])
    case.after(g, two_calls(g), setup)
    assert g.tick == case.ticks
    same_trackers(g, ids, ref["trackers"], case.what)
    same_reads(g, ref["reads"], case.what)
    same_answers(case.answers(g, setup), ref["end"], case.what)
    g.close()


# ---- 1. observers started on a restored handle ----
@pytest.mark.parametrize("fan,T", rs.DEEP_CASES)
def test_deep_started_on_a_restored_handle(hiplib, fan, T):
    case, img, cond, ref = rs.deep_run(fan, T)
    rs.check_deep(fan, T, cond, ref)
    carry_and_compare(case, resumed(case, img), ref)


def test_a_first_tick_that_has_passed_is_the_restored_tick(hiplib):
    """Samplers started behind the restore with a first tick long past and period 4: T, T + 4, ..."""
    case, img, cond, ref = rs.deep_run("krandomnodes", rs.DEEP_ODD, True)
    rs.check_passed(rs.DEEP_ODD, ref)
    carry_and_compare(case, resumed(case, img), ref)


@pytest.mark.parametrize("T", sorted(rs.SLOTS_T))
def test_slots_started_on_a_restored_handle(hiplib, T):
    case, img, cond, ref = rs.slots_run(T)
    rs.check_slots(T, cond, ref)
    carry_and_compare(case, resumed(case, img), ref)


@pytest.mark.parametrize("fan", sorted(sh.FANOUTS))
@pytest.mark.parametrize("n", rs.RESUME_SIZES)
def test_ragged_started_on_a_restored_handle(hiplib, n, fan):
    case, img, cond, ref = rs.ragged_run(n, fan)
    rs.check_ragged(n, fan, cond, ref)
    carry_and_compare(case, resumed(case, img), ref)


def test_lazy_planes_started_on_a_restored_handle(hiplib):
    """128 Ki nodes: the restored handle has memory for the view planes of the image's slots and for the ring planes of the
    clocks in its rows; the ledger's and the tracker's identity lies beyond them."""
    case = rs.lazy_case()
    g = create_lazy(hiplib, False, **case.kw)
    r0 = g.resident_planes()
    if r0["view"][0] == r0["view"][1]:
        pytest.skip("the mapping granularity of this device does not divide a plane of 128 Ki nodes: nothing is lazy here")
    ref = rs.lazy_reference()
    img, cond = case.image()
    rs.check_lazy(cond, ref)
    resumed(case, img, g)
    del img
    r1 = g.resident_planes()
    # Memory comes in chunks (serf_sim_host.inc lazy_reserve: 128 MiB at a time, an eighth of the array at most), so the image's
    # slots take whole chunks and no more.  The chunk is the eighth as long as an eighth of the planes stays below 128 MiB: 64 view
    # planes in two halves of 2 MiB here — asserted, so that another KW cannot make the shortcut wrong in silence.
    assert r1["view"][1] == 64 and r1["bytes_per_plane"] == 4 << 20 and (r1["view"][1] // 8) * (r1["bytes_per_plane"] // 2) <= 128 << 20
    chunk = r1["view"][1] // 8
    assert r1["view"][0] == -(-cond["n_slots"] // chunk) * chunk < r1["view"][1], (r1, cond["n_slots"])
    ahead = ref["setup"]["asked"][2]
    assert r1["event_ring"][0] <= ahead[2] % case.kw["event_ring"] < r1["event_ring"][1], "the identity's ring plane has memory already"
    carry_and_compare(case, g, ref)


# ---- 2. the `_now` entry points on a handle that has just been restored ----
def just_restored():
    return [("deep", fan, T) for fan, T in rs.DEEP_CASES] + [("slots", None, 101)]


@pytest.mark.parametrize("scenario,fan,T", just_restored())
def test_now_on_a_handle_that_has_just_been_restored(hiplib, scenario, fan, T):
    case, img, cond, ref = rs.deep_run(fan, T) if scenario == "deep" else rs.slots_run(T)
    g = resumed(case, img)
    same_now(g, ref["setup"], ref["now"][T], f"{case.what} right after the restore")
    g.step(1)
    same_now(g, ref["setup"], ref["now"][T + 1], f"{case.what} one step later")
    g.close()


# ---- 3. observers that exist before sim_restore ----
def test_observers_that_exist_before_a_restore(hiplib):
    ref = rs.before_reference()
    rs.check_before(ref)
    entries, asked = rs.deep_entries("krandomnodes")
    case, img, _, _ = rs.deep_run("krandomnodes", rs.BEFORE_T)
    g = serf_amd.create(case.n, **case.kw)
    start(g, rs.before_plan(entries))
    ids = add(g, rs.before_specs(entries))
    resumed(case, img, g)
    two_calls(g)(case.ticks - case.T)
    same_trackers(g, ids, ref["trackers"], "observers before a restore")
    same_reads(g, ref["reads"], "observers before a restore")
    same_answers(rs.abi_answers(g, asked), ref["end"], "observers before a restore")
    g.close()


# ---- 4. a snapshot in the middle of an observed run ----
def test_snapshots_in_the_middle_of_an_observed_run(hiplib):
    case, _, cond, ref = rs.deep_run("krandomnodes", 0)
    rs.check_deep("krandomnodes", 0, cond, ref)
    setup = ref["setup"]
    g = serf_amd.create(case.n, **case.kw)
    case.before(g)
    start(g, setup["plan"])
    ids = add(g, setup["specs"])
    seen = rs.snapshots_script(g, g.step, lambda: g.census_now(64))
    for got, model, name in zip(seen, ref["now"][rs.CENSUS_NOW_AT][1][0], ("header", "records")):
        same_words(got, model, f"census_now at tick {rs.CENSUS_NOW_AT}: {name}")
    assert g.tick == tl.DEEP_TICKS
    same_trackers(g, ids, ref["trackers"], "snapshots in the middle")
    same_reads(g, ref["reads"], "snapshots in the middle")
    same_answers(case.answers(g, setup), ref["end"], "snapshots in the middle")
    g.close()
