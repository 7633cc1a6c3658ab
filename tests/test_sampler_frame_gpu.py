"""The four periodic observers (series, census, roll, ledger) on ONE handle, each with its own (first_tick, period, capacity): what they
share — when a sample is due, where it goes, what a full buffer drops, what stop and a second start do — must stay each observer's own.
No model and no oracle: the sampled ticks follow from an observer's three numbers in plain Python (`rule`), and an observer that another
one's start, stop or restart leaves alone must read word for word what it read before."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi

pytestmark = pytest.mark.gpu

N, CRASHED, EVENT_NODE, EVENT_KEY = 300, 17, 5, 0x5A       # 300 nodes: one full workgroup and a ragged one
KW = dict(fanout=3, view_slots=32, event_ring=32, query_ring=16, probe_interval=2, suspicion_mult=3, suspicion_max_mult=2)
MAX_SUBJECTS, TOP_K, RANK_BY = 8, 4, _ffi.ROLL_BY_ACCUSED


def rule(started_at, first, period, capacity, now):
    """(the tick words of the samples held, (taken, dropped)) of an observer started at tick `started_at`, the handle now at `now`."""
    due = list(range(max(first, started_at), now, period))   # (a first tick that has passed means "now")
    return [t + 1 for t in due[:capacity]], (min(len(due), capacity), max(0, len(due) - capacity))


def parts(read):
    return (read,) if isinstance(read, np.ndarray) else tuple(read)   # (a series reads as one array, the others as headers and records)


def state(g, name):
    """(count, the complete read as bytes, its tick column) of a running observer."""
    read = parts(getattr(g, name + "_read")())
    return getattr(g, name + "_count")(), [np.ascontiguousarray(a).tobytes() for a in read], read[0]["tick"].tolist()


def check(g, running, now, what):
    """Every running observer follows its own rule: `running` maps name -> (started_at, first, period, capacity)."""
    for name, (started_at, first, period, capacity) in running.items():
        ticks, count = rule(started_at, first, period, capacity, now)
        got_count, _, got_ticks = state(g, name)
        print(f"{what}: {name} count {got_count} ticks {got_ticks}")
        assert got_count == count and got_ticks == ticks, f"{what}: {name} has {got_count} {got_ticks}, its rule says {count} {ticks}"


def gone(g, name):
    assert getattr(g, name + "_count")() == (0, 0)
    with pytest.raises(_ffi.SimError) as ei:
        getattr(g, name + "_read")(0, 0)
    assert ei.value.code == _ffi.ESTATE


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def test_four_samplers_keep_their_own_books(hiplib):
    g = serf_amd.create(N, **KW)
    entries = [(_ffi.K_EVENT, EVENT_KEY, g.stats(EVENT_NODE).event_time), (_ffi.K_DEAD, CRASHED, 0)]
    g.inject(0, _ffi.OP_CRASH, CRASHED)
    g.user_event(EVENT_NODE, EVENT_KEY, 64)
    # a buffer that fills (series), one behind every tick (census), a first tick in the future (roll), a period that ends on the last tick (ledger)
    running = {"series": (0, 3, 4, 6), "census": (0, 0, 1, 64), "roll": (0, 50, 3, 5), "ledger": (0, 11, 7, 8)}
    g.series_start(*running["series"][1:])
    g.census_start(*running["census"][1:], MAX_SUBJECTS)
    g.roll_start(*running["roll"][1:], TOP_K, RANK_BY)
    g.ledger_start(entries, *running["ledger"][1:])
    g.step(40)
    check(g, running, 40, "all four")
    assert rule(*running["series"], 40)[1] == (6, 4) and rule(*running["roll"], 40)[1] == (0, 0)   # (the cases meant above)
    # *_now with a running observer's parameters, all four live: its last sample, taken behind the last tick
    ch, cr = g.census_read()
    hdr, rec = g.census_now(MAX_SUBJECTS)
    assert int(ch["tick"][-1]) == 40 and same(hdr, ch[-1]) and same(rec, cr[-1][:int(ch["stored"][-1])])
    lh, lr = g.ledger_read()
    hdr, rec = g.ledger_now(entries)
    assert int(lh["tick"][-1]) == 40 and same(hdr, lh[-1]) and same(rec, lr[-1])
    assert int(ch["subjects"][-1]) > 0 and int(lr["reach"][-1][0]) > 1, "the census saw no subject / the event reached nobody"
    # stop in another order than they were started: the census while the roll runs, then the series
    for name in ("census", "series"):
        others = [o for o in running if o != name]
        before = {o: state(g, o) for o in others}
        getattr(g, name + "_stop")()
        del running[name]
        gone(g, name)
        for o in others:
            assert state(g, o) == before[o], f"{o} changed when the {name} stopped"
    # the census again, with other parameters, next to the roll and the ledger: its samples start at 0 under the new rule
    running["census"] = (40, 0, 2, 4)
    g.census_start(*running["census"][1:], MAX_SUBJECTS - 3)
    g.step(20)
    check(g, running, 60, "census restarted")
    assert rule(*running["census"], 60) == ([41, 43, 45, 47], (4, 6)) and rule(*running["roll"], 60)[0] == [51, 54, 57, 60]
    assert g.census_read()[1].shape == (4, MAX_SUBJECTS - 3)
    gone(g, "series")
    rh, rr = g.roll_read()
    hdr, top = g.roll_now(TOP_K, RANK_BY)
    assert same(hdr, rh[-1]) and same(top, rr[-1])
    before = {o: state(g, o) for o in ("census", "roll")}
    g.ledger_stop()
    gone(g, "ledger")
    assert {o: state(g, o) for o in ("census", "roll")} == before
    g.close()   # (the census and the roll still run)
