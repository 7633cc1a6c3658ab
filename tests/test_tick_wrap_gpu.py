"""The HIP library with the tick across its wrap points (the cases of tests/test_tick_wrap.py, which says what wraps and why).

Every handle here starts at a high tick: a fresh handle restored from the image of a fresh oracle whose tick the oracle's hook set
(tests/tick_wrap.py).  Across 2^21 the sites that form an age modulo 2^21 run with now < stamp:
  * against the third model, which does not wrap (the handlers' sites and join_sync_kernel),
  * against the oracle, full state, where the third model cannot follow (sparse views, recycling, virtual shards, deep queues,
    the two gossip_to_the_dead kernels), a checkpoint taken three ticks before the wrap included,
  * the observers that store ticks (trackers, detection log, spread map) beside such a run, against their models on the oracle.
At SIM_TICK_MAX: the run that ends there equals the oracle's and the third model's, and what lies beyond is refused as the
oracle refuses it.  Every comparison is exact."""
import pytest

from serf_amd import _ffi
from tests import _scenario as sc
from tests import test_ledger as tl
from tests import test_parity_gpu as tp
from tests import test_tick_wrap as tw
from tests.detect_model import DetectModel
from tests.spread_model import SpreadModel
from tests.test_detect_gpu import assert_same as detect_same
from tests.test_spread import event_ltimes
from tests.test_spread_gpu import same_reads as spread_same_reads, same_samples as spread_same_samples
from tests.test_track_gpu import FAILED, KRANDOM, SUSPECT_OR_DEAD, assert_same as track_same
from tests.tick_wrap import WRAP, shifted, started_at
from tests.track_model import TrackModel

pytestmark = pytest.mark.gpu
T0 = WRAP - 24


# ---- 1. against the third model ----
@pytest.mark.parametrize("name", ("layer 0", "reaper 1", "switches 3", "prune", "join_sync"))
def test_hip_matches_the_third_model_across_2_21(oracle, hiplib, name):
    got = tw.run_case(hiplib, oracle, name, T0)
    for what in tw.STRADDLES[name, T0]:
        assert got[what] > 0, f"{name}: nothing of `{what}` reached across the wrap ({got})"


# ---- 2. against the oracle, full state ----
# The seeds with the SWIM layer on among the first 16 of each of tests/test_parity_gpu.py's two sweeps, and what each brings
# (gttd: gossip_to_the_dead > 0; v4: vshards == 4; pkt: pkt_records >= 8):
#   test_random_configurations (the bijection):  0 recycle | 2 join_sync recycle | 3 gttd join_sync reap | 5 gttd reap |
#     6 join_sync reap | 9 join_sync reap | 10 gttd reap | 11 join_sync reap | 12 reap | 13 gttd join_sync | 14 gttd reap |
#     15 join_sync recycle
#   test_random_fanout_kRandomNodes:  1 gttd join_sync recycle | 2 gttd recycle | 3 gttd join_sync | 4 recycle |
#     5 join_sync reap | 6 v4 | 7 join_sync recycle | 8 gttd join_sync reap | 9 gttd join_sync | 10 gttd reap | 11 gttd |
#     12 gttd join_sync recycle | 15 gttd reap v4
# No seed below 16 has packets of more than one page (the fan-out sweep draws them from seed 16 on), and none of the
# bijection's has virtual shards with the SWIM layer on: kRandomNodes seed 21 (pkt 16, gttd, join_sync, recycling, 1 000 nodes)
# and bijection seed 20 (v4, gttd, join_sync, reap, recycling, 4 096 nodes) are added for them.
BIJECTION_SEEDS = (0, 2, 3, 5, 6, 9, 10, 11, 12, 13, 14, 15, 20)
KRANDOM_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 21)
SWEEPS = [("bijection", s) for s in BIJECTION_SEEDS] + [("krandomnodes", s) for s in KRANDOM_SEEDS]


def sweep_configuration(sweep, seed):
    return (tp.random_configuration if sweep == "bijection" else tp.random_fanout_configuration)(seed)


def test_the_seeds_are_the_sweeps_swim_seeds_and_cover_every_knob():
    drawn = {(sweep, seed): sweep_configuration(sweep, seed)[1] for sweep, seed in SWEEPS}
    for sweep, seeds in (("bijection", BIJECTION_SEEDS), ("krandomnodes", KRANDOM_SEEDS)):
        assert [s for s in range(16) if sweep_configuration(sweep, s)[1]["probe_interval"]] == [s for s in seeds if s < 16]
    assert all(kw["probe_interval"] for kw in drawn.values())
    rf = lambda kw: bool(kw.get("flags", _ffi.CF_BASELINE_JOINED) & _ffi.CF_RANDOM_FANOUT)
    for what, has in (("gossip_to_the_dead with kRandomNodes (rf_skip_kernel)", lambda kw: kw["gossip_to_the_dead"] > 0 and rf(kw)),
                      ("gossip_to_the_dead with the bijection (gossip_skip_kernel)", lambda kw: kw["gossip_to_the_dead"] > 0 and not rf(kw)),
                      ("join_sync", lambda kw: kw["join_sync"]), ("reap_interval", lambda kw: kw["reap_interval"] > 0),
                      ("recycle_interval", lambda kw: kw["recycle_interval"] > 0), ("vshards == 4", lambda kw: kw.get("vshards") == 4),
                      ("pkt_records >= 8", lambda kw: kw.get("pkt_records", 0) >= 8)):
        assert any(has(kw) for kw in drawn.values()), what


@pytest.mark.parametrize("sweep,seed", SWEEPS)
def test_hip_matches_the_oracle_across_2_21(oracle, hiplib, sweep, seed):
    n, kw, rate, dense = sweep_configuration(sweep, seed)
    g, o = started_at(hiplib, oracle, n, T0, **kw), started_at(oracle, oracle, n, T0, **kw)
    members = (12 if not dense else min(n // 2, 30)) if sweep == "bijection" else max(1, min(n // 2, 12 if not dense else 30))
    ops = shifted(sc.schedule(n, 40, rate=rate, seed=seed, max_member_subjects=members), T0)
    sc.apply_schedule(g, ops)
    sc.apply_schedule(o, ops)
    for t in range(T0, T0 + 64):
        g.step(1)
        o.step(1)
        if g.digest() != o.digest():
            sc.assert_same_state(g, o, f"{sweep} seed {seed} n={n} {kw} tick {t}")
            raise AssertionError(f"digest differs after tick {t} but the arrays agree")
    sc.assert_same_state(g, o, f"{sweep} seed {seed} final")
    assert g.cluster_stats()["ops_dropped"] == o.cluster_stats()["ops_dropped"]
    g.close(); o.close()


def test_deep_queues_across_2_21(oracle, hiplib):
    # tests/test_ledger.py's DEEP scenario: 512 nodes, packets of two pages, queues beyond SIM_Q_HOT (deep_queue_kernel) — from
    # 2^21 - 31, so that the ticks with the deepest queues lie on both sides of the wrap
    D0 = WRAP - 31
    g, o = started_at(hiplib, oracle, tl.DEEP_N, D0, **tl.DEEP_KW), started_at(oracle, oracle, tl.DEEP_N, D0, **tl.DEEP_KW)
    ops = shifted(sc.schedule(tl.DEEP_N, 40, rate=2.0, seed=524, max_member_subjects=40), D0)       # deep_drive's schedule
    sc.apply_schedule(g, ops)
    sc.apply_schedule(o, ops)
    deepest = {}
    for t in range(D0, D0 + tl.DEEP_TICKS):
        g.step(1)
        o.step(1)
        assert g.digest() == o.digest(), f"digest differs after tick {t}"
        deepest[t] = int((o.dump(_ffi.ARR_QUEUE).reshape(tl.DEEP_N, _ffi.Q)["meta"] != 0xFFFFFFFF).sum(axis=1).max())
    sc.assert_same_state(g, o, "deep queues, final")
    # (on the oracle's dump) queues deeper than the kernel's registers hold on both sides of the wrap
    assert max(d for t, d in deepest.items() if t < WRAP) > _ffi.Q_HOT and max(d for t, d in deepest.items() if t >= WRAP) > _ffi.Q_HOT
    g.close(); o.close()


def test_a_checkpoint_three_ticks_before_the_wrap(oracle, hiplib):
    n, kw, C0 = tw.ROUTE_N, tw.ROUTE_KW, WRAP - 40
    g, o = started_at(hiplib, oracle, n, C0, **kw), started_at(oracle, oracle, n, C0, **kw)
    ops = shifted(sc.schedule(n, 60, rate=0.9, seed=77, max_member_subjects=30), C0)
    sc.apply_schedule(g, ops)
    sc.apply_schedule(o, ops)
    g.step(37)
    o.step(37)
    assert g.tick == o.tick == WRAP - 3
    gi, oi = g.snapshot(), o.snapshot()
    assert bytes(gi) == bytes(oi), "the two images taken at 2^21 - 3 differ"
    g2, o2 = _ffi.Sim(hiplib, _ffi.make_config(n, **kw)), _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    g2.restore(oi)
    o2.restore(gi)
    assert g2.tick == o2.tick == WRAP - 3
    for t in range(30):
        for s in (g, o, g2, o2):
            s.step(1)
        assert g.digest() == o.digest() == g2.digest() == o2.digest(), f"digests differ after tick {WRAP - 3 + t}"
    sc.assert_same_state(g2, o2, "restored across the wrap")
    sc.assert_same_state(g2, o, "restored against the run that went on")
    for s in (g, o, g2, o2):
        s.close()


# ---- 3. the observers that store ticks ----
OBS_N, OBS_TICKS = 257, 64
OBS_KW = dict(fanout=3, view_slots=32, event_ring=64, query_ring=64, probe_interval=2, suspicion_mult=3, suspicion_max_mult=2, loss=0.01,
              ring_overflow=4, flags=KRANDOM)
OBS_CRASHES = ((3, 200), (9, 31), (15, 256), (22, 64), (30, 129))      # (tick after T0, node): before, at and after the wrap
OBS_EVENTS = tuple((2 + 5 * i, (37 * i + 5) % 190, 0x52000000 + i) for i in range(10))      # (tick after T0, origin, key)


def obs_script(sim, step):
    for t, x in OBS_CRASHES:
        sim.inject(T0 + t, _ffi.OP_CRASH, x)
    for t, x, key in OBS_EVENTS:
        sim.inject(T0 + t, _ffi.OP_USER_EVENT, x, key, 64)
    step(OBS_TICKS)


def obs_trackers(entries):
    specs = []
    for t, x in OBS_CRASHES:
        specs.append(_ffi.member_tracker(x, FAILED, SUSPECT_OR_DEAD, start=T0 + t))
        specs.append(_ffi.member_tracker(x, FAILED, start=T0 + t, max_age=40))
    specs.append(_ffi.member_tracker(7, FAILED, SUSPECT_OR_DEAD))                          # a node that keeps running
    for (kind, key, ltime), (t, _, _) in zip(entries, OBS_EVENTS):
        specs.append(_ffi.rumour_tracker(kind, key, ltime, start=T0 + t if key & 1 else 0, max_age=30 if key & 2 else 0))
    return specs


def test_trackers_detection_log_and_spread_map_across_2_21(oracle, hiplib):
    make = lambda: started_at(oracle, oracle, OBS_N, T0, **OBS_KW)
    lts = event_ltimes(make, obs_script)
    entries = [(_ffi.K_EVENT, key, lts[key]) for _, _, key in OBS_EVENTS]
    # the models on the oracle, one tick at a time
    o = make()
    track, detect, spread = TrackModel(o), DetectModel(o), SpreadModel(o)
    hs = [track.add(s) for s in obs_trackers(entries)]
    detect.start(0, 1, OBS_TICKS)
    spread.start(entries, 0, 1, OBS_TICKS)

    def model_step(k):
        for _ in range(k):
            t = o.tick
            o.step(1)
            track.evaluate()
            detect.after_tick(t)
            spread.after_tick(t)
    obs_script(o, model_step)
    want = [track.result(h) for h in hs]
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    # what the run is for: ticks on both sides of the wrap in every observer's results
    both_sides = lambda ticks: min(ticks) < WRAP <= max(ticks)
    assert both_sides([r["first"] for r in want if r["first"] != _ffi.TRACK_NEVER])
    wl = detect.log()
    assert len(wl) and both_sides(list(wl["opened"]) + list(wl["closed"]))
    assert both_sides([int(a) for a in spread.arrival[spread.arrival != 0]])
    # the library, in one long call
    g = started_at(hiplib, oracle, OBS_N, T0, **OBS_KW)
    ids = g.track_add(obs_trackers(entries))
    g.detect_start(0, 1, OBS_TICKS)
    g.spread_start(entries, capacity=OBS_TICKS)
    obs_script(g, g.step)
    track_same([r.as_dict() for r in g.track_read(ids)], want, "trackers across 2^21")
    assert g.detect_count() == detect.count() == (OBS_TICKS, 0) and g.detect_log_count() == detect.log_count()
    detect_same(g, (detect.read(), wl, detect.open()), "detection log across 2^21")
    assert g.spread_count() == spread.count() == (OBS_TICKS, 0)
    spread_same_samples(g.spread_read(), spread.read(), "spread map across 2^21")
    spread_same_reads(g, spread, "spread map across 2^21", top_ks=(7,))
    assert g.digest() == o.digest()
    g.close(); o.close()


# ---- 4. the tick limit ----
@pytest.mark.parametrize("name", tw.LIMIT_CASES)
def test_a_run_that_ends_at_the_last_tick_matches_the_oracle_and_the_third_model(oracle, hiplib, name):
    g = tw.check_run_to_the_limit(hiplib, oracle, name)
    o = tw.check_run_to_the_limit(oracle, oracle, name)
    assert g.digest() == o.digest()
    sc.assert_same_state(g, o, f"{name} behind SIM_TICK_MAX")
    g.close(); o.close()


def test_a_step_beyond_the_last_tick_is_refused_whole(oracle, hiplib):
    g, o = tw.check_whole_step_is_checked_first(hiplib, oracle), tw.check_whole_step_is_checked_first(oracle, oracle)
    assert g.digest() == o.digest()
    g.close(); o.close()


def test_an_image_beyond_the_last_tick_is_refused(oracle, hiplib):
    g, o = tw.check_image_beyond_the_limit(hiplib, oracle), tw.check_image_beyond_the_limit(oracle, oracle)
    assert g.digest() == o.digest()
    g.close(); o.close()


def test_create_refuses_intervals_an_age_cannot_reach(hiplib):
    tw.check_intervals(hiplib)
