"""The per-tick host path (serf_amd/csrc/serf_sim_step.inc) on the branches no other test runs, at the smallest shape where they are
live: one handle with the random fan-out whose request lists are in use — slot-less suspicions and reconnect attempts replayed two
ticks later —, a push-pull batch, gossip to the dead and loss.  Every case steps one tick at a time and must hold the oracle's digest
after every tick:
  default   no switch: the graphs are built two ticks ahead on the build stream, behind the stop event of the tick before
  sync      SERF_RF_SYNC=1: every graph is built on the handle's own stream when the tick that reads it begins
  timed     timing events on the tick's dispatch: the completion event of a tick is a timing event, the handle's own, or — right after
            the timing events were read and destroyed — none, and the builds then wait for a marker
  resumed   an image restored into a fresh handle: no graph is queued there, the first tick builds two on the spot
The condition that makes the shape meaningful — the request lists really are in use — is tested on the oracle alone, without a GPU."""
import pytest

import serf_amd
from serf_amd import _ffi
from tests import _scenario as sc
from tests._oracle import load_oracle

N, TICKS = 2048, 40
KW = dict(flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT, fanout=4, view_slots=32, event_ring=16, query_ring=8,
          probe_interval=2, loss=0.05, push_pull_interval=20, reconnect_interval=4, gossip_to_the_dead=1,
          suspicion_mult=3, suspicion_max_mult=2)


def scheduled(sim):
    sc.apply_schedule(sim, sc.schedule(N, 20, rate=1.0, seed=11, max_member_subjects=12))
    for node in range(30, N, 97):
        sim.inject(2, _ffi.OP_CRASH, node)
    return sim


def new_oracle():
    return scheduled(_ffi.Sim(load_oracle(), _ffi.make_config(N, **KW)))


@pytest.fixture(scope="module")
def want():
    """The oracle's digest after each of the TICKS ticks, stepped one at a time (computed once for the module, never changed)."""
    o = new_oracle()
    out = []
    for _ in range(TICKS):
        o.step(1)
        out.append(o.digest())
    o.close()
    return tuple(out)


def run(g, want, first, last):
    for t in range(first, last):
        g.step(1)
        assert g.digest() == want[t], f"the HIP path left the oracle in tick {t}"


def test_request_lists_are_in_use():
    """A probe oracle (reading a list consumes it, so its digests are nobody's reference) sees a non-empty request list after at least
    10 of the 40 ticks.  Measured: 29 of 40, lists of 1 to 13 pairs, no operation dropped."""
    p = new_oracle()
    sizes = []
    for _ in range(TICKS):
        p.step(1)
        sizes.append(len(p.suspect_requests()))
    used = [s for s in sizes if s]
    print(f"request lists: non-empty after {len(used)} of {TICKS} ticks, {min(used, default=0)} to {max(used, default=0)} pairs, "
          f"ops_dropped {p.cluster_stats()['ops_dropped']}")
    p.close()
    assert len(used) >= 10


@pytest.mark.gpu
def test_default(hiplib, want):
    g = scheduled(serf_amd.create(N, **KW))
    run(g, want, 0, TICKS)
    g.close()


@pytest.mark.gpu
def test_sync(hiplib, want, monkeypatch):
    monkeypatch.setenv("SERF_RF_SYNC", "1")   # (read when the handle is created)
    g = scheduled(serf_amd.create(N, **KW))
    run(g, want, 0, TICKS)
    g.close()


@pytest.mark.gpu
def test_timed(hiplib, want):
    g = scheduled(serf_amd.create(N, **KW))
    g.profile(1)
    run(g, want, 0, 13)
    assert g.profile_read_stats()[1] == 13
    run(g, want, 13, 14)   # (the tick behind a read has no completion event of the tick before it: a marker)
    assert g.profile_read_stats()[1] == 1
    g.profile(3)           # (and this one; from here on every third tick's completion event is a timing event)
    run(g, want, 14, TICKS)
    assert g.profile_read_stats()[1] == -(-(TICKS - 14) // 3)
    g.close()


@pytest.mark.gpu
def test_resumed(hiplib, want):
    g = scheduled(serf_amd.create(N, **KW))
    run(g, want, 0, 17)
    fresh = serf_amd.create(N, **KW)
    fresh.restore(g.snapshot())
    for t in range(17, TICKS):
        g.step(1)
        fresh.step(1)
        assert g.digest() == fresh.digest() == want[t], f"tick {t}: original, restored handle and oracle disagree"
    g.close()
    fresh.close()
