"""The tick across its wrap points, the part that needs no GPU.

A view entry's stamp is the tick in 21 bits and every age is (now - stamp) & 0x1FFFFF, so a run that crosses tick 2^21 forms ages
with now < stamp; deadlines are 32-bit sums, so ticks end at SIM_TICK_MAX = 2^32 - 2^22 - 1 (include/serf_sim.h).  Here:

  * the oracle against the third model (tests/third_model_swim.py: Python integers, no wrap) from 2^21 - 40 and 2^21 - 24, with a
    condition per case — computed on the model alone — that state did reach across the wrap,
  * the two routes to a high tick (the oracle's hook, an image) against each other,
  * the tick limit: a run whose last tick is SIM_TICK_MAX agrees with the third model, a step beyond it is SIM_ERANGE and changes
    nothing, an image beyond it is SIM_EINVAL on a handle that stays fresh, and sim_create refuses intervals >= 2^21.

This file owns the cases that tests/test_tick_wrap_gpu.py runs on the GPU as well.

Straddle counts of the model (suspicion-ticks / departed leave times / reaped intents; tests.tick_wrap.straddles), at 2^21 - 40
and 2^21 - 24:
  layer 0     350 /   0 / 0   and  196 /  60 / 0
  reaper 1    219 / 119 / 1   and  252 / 121 / 0
  switches 3   90 / 168 / 0   and  277 / 132 / 0
  prune        80 /   5 / 0   and  207 /   9 / 0
  join_sync   458 / 205 / 0   and  641 /  90 / 0
  burst       309 / 198 / 0   and  114 /  97 / 0
  switches 4  737 /  55 / 0   and  556 /   0 / 0
  sweep 3     144 / 234 / 0   and  391 / 132 / 0
  sweep 7     314 /   0 / 0   and  790 /   0 / 0
  sweep 9     144 /  82 / 0   and    0 /   0 / 0
A count of 0 is a property of that schedule (nobody leaves or fails early enough, or everybody suspected before the wrap is
settled by it); STRADDLES asserts every other one as > 0."""
import pytest

from serf_amd import _ffi
from tests import _scenario as sc
from tests import test_third_model_swim as t3
from tests.tick_wrap import WRAP, image_at, shifted, started_at, straddles

T0S = (WRAP - 40, WRAP - 24)


def _kw(fanout, loss, pi, **more):
    return dict(t3.KW, fanout=fanout, loss=loss, probe_interval=pi, **more)


def case(name):
    """(n, kw, ops, ticks) of a named third-model case: the configurations and schedules of tests/test_third_model_swim.py."""
    if name == "layer 0":
        seed, n, fanout, loss, pi = t3.CASES[0]
        return n, _kw(fanout, loss, pi), t3._schedule(n, 110, seed), 110
    if name == "reaper 1":
        seed, n, fanout, loss, pi, ppi = t3.REAP_CASES[1]
        return n, _kw(fanout, loss, pi, push_pull_interval=ppi, **t3.REAP_KW), t3._schedule(n, 110, seed), 110
    if name in ("switches 3", "switches 4"):
        seed, n, fanout, loss, pi, sw = t3.SWITCH_CASES[int(name[-1])]
        ops = t3._resume_schedule(n, 110, seed) if name == "switches 3" else t3._schedule(n, 110, seed)   # (3: gossip_to_the_dead + Reconnector)
        return n, _kw(fanout, loss, pi, **sw), ops, 110
    if name == "prune":
        seed, n, fanout, loss, pi, delay = t3.PRUNE_CASES[0]
        kw = _kw(fanout, loss, pi, leave_delay=delay, prune_delay=True, reap_interval=6, reconnect_timeout=60, tombstone_timeout=60)
        return n, kw, t3._prune_schedule(n, 120, seed), 120
    if name == "join_sync":
        seed, n, fanout, loss, pi = 91, 48, 3, 0.03, 2
        return n, _kw(fanout, loss, pi, join_sync=True, tcp_fallback=True), t3._rejoin_schedule(n, 110, seed), 110
    if name == "burst":
        seed, n, fanout, loss, pi = 41, 48, 3, 0.02, 2
        return n, _kw(fanout, loss, pi, push_pull_interval=0, **t3.QC_KW, **t3.REAP_KW), t3._burst_schedule(n, 110, seed), 110
    assert name.startswith("sweep ")
    n, kw, ops = t3._sweep_case(int(name[6:]))
    return n, kw, ops, 110


CASES = ("layer 0", "reaper 1", "switches 3", "prune", "join_sync", "burst", "switches 4", "sweep 3", "sweep 7", "sweep 9")
# Which straddle counts must be > 0, per case and start: the counts of the MODEL alone (they never depend on the code under test).
# The first six cases have suspicions and leave times across the wrap from both starts, but for "layer 0" from 2^21 - 40, where
# no leave time written below the wrap goes away above it; "reaper 1" from 2^21 - 40 is the one run in which the Reaper erases a
# buffered intent stamped below the wrap.  The other four as the model has them (the table in this file's docstring).
STRADDLES = {(name, T0): ("susp", "left") for name in CASES for T0 in T0S}
STRADDLES["layer 0", WRAP - 40] = ("susp",)
STRADDLES["reaper 1", WRAP - 40] = ("susp", "left", "intents")
STRADDLES["switches 4", WRAP - 24] = ("susp",)
STRADDLES["sweep 7", WRAP - 40] = STRADDLES["sweep 7", WRAP - 24] = ("susp",)
STRADDLES["sweep 9", WRAP - 24] = ()


def run_case(lib, oracle, name, T0):
    """The named case from tick T0 on a handle of `lib`, against the third model after every tick; returns the model's straddle counts."""
    n, kw, ops, ticks = case(name)
    sim = started_at(lib, oracle, n, T0, **kw)
    with straddles() as got:
        t3.run(sim, n, ops, ticks, True, t0=T0, **kw)
    assert sim.tick == T0 + ticks
    sim.close()
    return got


@pytest.mark.parametrize("T0", T0S)
@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_the_third_model_across_2_21(oracle, name, T0):
    got = run_case(oracle, oracle, name, T0)
    print(f"straddles {name} from 2^21 - {WRAP - T0}: {got}")
    for what in STRADDLES[name, T0]:
        assert got[what] > 0, f"{name} from {T0}: nothing of `{what}` reached across the wrap ({got})"


# ---- the two routes to a high tick ----
ROUTE_N = 1024
ROUTE_KW = dict(fanout=4, view_slots=64, event_ring=16, query_ring=8, leave_delay=6, probe_interval=3, loss=0.02, push_pull_interval=8,
                reap_interval=7, reconnect_timeout=25, tombstone_timeout=40, intent_timeout=20, recycle_interval=6,
                flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT)


def test_the_hook_and_the_image_lead_to_the_same_run(oracle):
    T0 = WRAP - 40
    a = _ffi.Sim(oracle, _ffi.make_config(ROUTE_N, **ROUTE_KW))
    assert oracle.t["set_tick"](a.h, T0) == 0
    b = started_at(oracle, oracle, ROUTE_N, T0, **ROUTE_KW)
    ops = shifted(sc.schedule(ROUTE_N, 60, rate=0.9, seed=77, max_member_subjects=30), T0)
    sc.apply_schedule(a, ops)
    sc.apply_schedule(b, ops)
    assert a.digest() == b.digest()
    for t in range(80):
        a.step(1)
        b.step(1)
        assert a.digest() == b.digest(), f"the routes differ after tick {T0 + t}"
    sc.assert_same_state(a, b, "hook against image")
    assert a.tick == b.tick == T0 + 80 and a.cluster_stats()["slots_recycled"] > 0


# ---- the tick limit ----
LIMIT_CASES = ("layer 0", "reaper 1")
INTERVALS = ("probe_interval", "intent_timeout", "leave_delay", "reap_interval", "reconnect_timeout", "tombstone_timeout",
             "queue_check_interval", "push_pull_interval", "recycle_interval", "gossip_to_the_dead", "reconnect_interval")
SMALL_KW = dict(fanout=3, view_slots=16, event_ring=8, query_ring=8, probe_interval=2)


def check_refused_step(sim, n_ticks=1):
    """sim_step(n_ticks) is SIM_ERANGE and leaves tick and digest as they were"""
    tick, digest = sim.tick, sim.digest()
    with pytest.raises(_ffi.SimError) as ei:
        sim.step(n_ticks)
    assert ei.value.code == _ffi.ERANGE
    assert (sim.tick, sim.digest()) == (tick, digest)


def check_run_to_the_limit(lib, oracle, name):
    """110 ticks against the third model, the last of them SIM_TICK_MAX; the next step is refused, in one piece and begun by hand"""
    n, kw, ops, ticks = case(name)
    T0 = _ffi.TICK_MAX + 1 - ticks
    sim = started_at(lib, oracle, n, T0, **kw)
    t3.run(sim, n, ops, ticks, True, t0=T0, **kw)
    assert sim.tick == _ffi.TICK_MAX + 1
    check_refused_step(sim)
    digest = sim.digest()
    with pytest.raises(_ffi.SimError) as ei:
        sim.step_begin()
    assert ei.value.code == _ffi.ERANGE and sim.digest() == digest
    return sim


def check_whole_step_is_checked_first(lib, oracle):
    sim = started_at(lib, oracle, 64, _ffi.TICK_MAX - 3, **SMALL_KW)
    check_refused_step(sim, 5)              # its fifth tick would be SIM_TICK_MAX + 1: none of the five is executed
    sim.step(4)
    assert sim.tick == _ffi.TICK_MAX + 1
    check_refused_step(sim)
    sim.step(0)
    return sim


def check_image_beyond_the_limit(lib, oracle):
    fresh = _ffi.Sim(lib, _ffi.make_config(64, **SMALL_KW))
    digest = fresh.digest()
    for T0 in (_ffi.TICK_MAX + 1, 2 ** 32 - 40, 2 ** 32 + 5):
        with pytest.raises(_ffi.SimError) as ei:
            fresh.restore(image_at(oracle, 64, T0, **SMALL_KW))
        assert ei.value.code == _ffi.EINVAL
        assert fresh.tick == 0 and fresh.digest() == digest
    fresh.restore(image_at(oracle, 64, _ffi.TICK_MAX, **SMALL_KW))      # still fresh: it takes an image, the last tick's
    fresh.step(1)
    check_refused_step(fresh)
    return fresh


def check_intervals(lib, create=True):
    for name in INTERVALS:
        kw = dict(SMALL_KW, **{name: _ffi.INTERVAL_LIMIT})
        with pytest.raises(_ffi.SimError) as ei:
            _ffi.Sim(lib, _ffi.make_config(64, **kw))
        assert ei.value.code == _ffi.EINVAL, name
        kw = dict(SMALL_KW, **{name: 0xFFFFFFFF})
        with pytest.raises(_ffi.SimError) as ei:
            _ffi.Sim(lib, _ffi.make_config(64, **kw))
        assert ei.value.code == _ffi.EINVAL, name
        if create:
            _ffi.Sim(lib, _ffi.make_config(64, **dict(SMALL_KW, **{name: _ffi.INTERVAL_LIMIT - 1}))).close()
    # the suspicion table's largest entry stays below 2^21 whatever the multipliers (sim_create caps it at 2 000 000)
    if create:
        _ffi.Sim(lib, _ffi.make_config(64, **dict(SMALL_KW, probe_interval=_ffi.INTERVAL_LIMIT - 1, suspicion_mult=40, suspicion_max_mult=60))).close()


@pytest.mark.parametrize("name", LIMIT_CASES)
def test_a_run_that_ends_at_the_last_tick_matches_the_third_model(oracle, name):
    check_run_to_the_limit(oracle, oracle, name).close()


def test_a_step_beyond_the_last_tick_is_refused_whole(oracle):
    check_whole_step_is_checked_first(oracle, oracle).close()


def test_the_run_that_diverged_at_2_32_is_refused(oracle):
    # 110 ticks from 2^32 - 40: the oracle left the third model at 2^32 - 19.  No handle gets there: the hook can put the tick
    # there, and the first step is refused
    n, kw, ops, ticks = case("layer 0")
    sim = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    assert oracle.t["set_tick"](sim.h, 2 ** 32 - 40) == 0
    sc.apply_schedule(sim, shifted(ops, 2 ** 32 - 40))
    check_refused_step(sim)
    check_refused_step(sim, ticks)
    sim.close()


def test_an_image_beyond_the_last_tick_is_refused(oracle):
    check_image_beyond_the_limit(oracle, oracle).close()


def test_create_refuses_intervals_an_age_cannot_reach(oracle):
    check_intervals(oracle)
