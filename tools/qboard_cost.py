#!/usr/bin/env python
"""What a sample of the query board (include/serf_sim_qboard.h) costs, beside a series sample of the same run and beside the polled
alternative it replaces — n x sim_query_status behind every tick (run on the GPU box).

usage: python tools/qboard_cost.py [--nodes N] [--entries 1,16,64] [--ticks 40] [--rounds 3] [--out FILE]
       python tools/qboard_cost.py --only qboard|series|polled|none [--n-entries 16] [--ticks 40]
                                   one kind of window, for a rocprofv3 --kernel-trace --stats run of its own

The handle is tools/census_cost.py's (1 Mi nodes, kRandomNodes, fan-out 4, SWIM on).  64 queries are issued, four a tick from random
nodes, a third of them filtered by id or by tag class, so that every entry is a query whose answers come in while the windows run.
Windows of `ticks` ticks alternate, `rounds` times, between
  none     ONE sim_step(ticks) ending in a synchronise
  series   the same with a series sample behind every tick
  qboard   the same with a board of k entries behind every tick
  polled   `ticks` x (sim_step(1), then sim_query_status of each of the k ids): two synchronisations, a launch and a copy per id and tick
and the differences of the medians to `none` are what each adds to a tick, end to end; the ranges of the rounds are printed with
them.  A board sample reads, per node, 16 B of its row and its tag-class byte, and per entry and wave of 64 nodes four words of the
bitmaps: the bytes by that count are printed next to the times.  The three reads (silent, nodes, top) are timed once at the end."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from census_cost import timed  # noqa: E402  (imports torch first: one HIP runtime per process)

import numpy as np  # noqa: E402

import serf_amd  # noqa: E402
from serf_amd import _ffi  # noqa: E402

QUERIES = 64


def median(x):
    return sorted(x)[len(x) // 2]


def spread(x):
    return [min(x), median(x), max(x)]


def make(n):
    kw = dict(fanout=4, view_slots=1024, event_ring=512, query_ring=512, probe_interval=5, push_pull_interval=150, loss=0.0,
              ring_overflow=8, join_sync=True, flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT)
    sim = serf_amd.create(n, **kw)
    sim.init_tags((np.arange(n) % 4).astype(np.uint8))
    return sim


def issue(sim, n, rng, ids):
    """The queries of one window: four a tick from random nodes from the next tick on; a third filtered."""
    t0 = sim.tick + 1
    for i, qid in enumerate(ids):
        node = int(rng.integers(n))
        flags = _ffi.F_ACK | (_ffi.F_RESPOND if i % 2 else 0) | ((i % 4) << 8)
        if i % 3 == 1:
            for x in rng.choice(n, 12, replace=False).tolist():
                sim.inject(t0 + i // 4, _ffi.OP_QUERY_FILTER_ID, node, qid, int(x))
        elif i % 3 == 2:
            sim.inject(t0 + i // 4, _ffi.OP_QUERY_FILTER_TAGS, node, qid, 0b0110)
        sim.inject(t0 + i // 4, _ffi.OP_QUERY, node, qid, flags)


def polled(sim, ids, ticks):
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(ticks):
        sim.step(1)
        for qid in ids:
            try:
                sim.query_status(qid)
            except _ffi.SimError:
                pass                     # (not running yet: the poll was made all the same)
    sim.sync()
    return (time.perf_counter() - t0) / ticks * 1e6


def timed_call(sim, fn):
    sim.sync()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--entries", default="1,16,64")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--n-entries", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.nodes
    rng = np.random.default_rng(3)
    sim = make(n)
    sim.step(4)
    serial = [0]

    def fresh_ids():
        """Ids nobody has used: every window follows queries that are being answered while it runs."""
        serial[0] += 1
        return [serial[0] * 1000 + i for i in range(QUERIES)]

    if a.only:
        ids = fresh_ids()
        issue(sim, n, rng, ids)
        es = ids[:a.n_entries]
        if a.only == "qboard":
            sim.qboard_start(es, 0, 1, a.ticks + 4)
        elif a.only == "series":
            sim.series_start(0, 1, a.ticks + 4)
        sim.step(2)
        us = polled(sim, es, a.ticks) if a.only == "polled" else timed(sim, a.ticks)
        print(json.dumps({"nodes": n, "only": a.only, "entries": len(es), "step_us": us}))
        return
    counts = [int(x) for x in a.entries.split(",")]
    out = {"nodes": n, "ticks": a.ticks, "rounds": a.rounds, "by_entries": {}}
    for k in counts:
        none, ser, brd, pol = [], [], [], []
        reads, last = {}, None
        for r in range(a.rounds):
            for kind in ("none", "series", "qboard", "polled"):
                ids = fresh_ids()
                issue(sim, n, rng, ids)
                es = ids[:k]
                if kind == "series":
                    sim.series_start(0, 1, a.ticks + 4)
                elif kind == "qboard":
                    sim.qboard_start(es, 0, 1, a.ticks + 4)
                sim.step(2)              # first launches
                if kind == "polled":
                    pol.append(polled(sim, es, a.ticks))
                else:
                    {"none": none, "series": ser, "qboard": brd}[kind].append(timed(sim, a.ticks))
                if kind == "series":
                    sim.series_stop()
                elif kind == "qboard":
                    hdr, rec = sim.qboard_read()
                    assert len(hdr) == a.ticks + 2
                    last = rec[-1]
                    if r + 1 == a.rounds:
                        reads = {"silent_us": timed_call(sim, lambda: sim.qboard_silent(0, 0, 64)),
                                 "nodes_us": timed_call(sim, lambda: sim.qboard_nodes()),
                                 "top64_us": timed_call(sim, lambda: sim.qboard_top(64)),
                                 "top64_nodes_us": timed_call(sim, lambda: sim.qboard_top(64, nodes=True)),
                                 "now_us": timed_call(sim, lambda: sim.qboard_now(es))}
                    sim.qboard_stop()
        mn = median(none)
        by = {"step_us_none": spread(none), "step_us_series": spread(ser), "step_us_qboard": spread(brd), "step_us_polled": spread(pol),
              "series_added_us_per_sample": median(ser) - mn, "qboard_added_us_per_sample": median(brd) - mn,
              "polled_added_us_per_tick": median(pol) - mn, "none_spread_us": max(none) - min(none),
              # per sample: 16 B of every node's row and its class byte; per entry and wave four words of the bitmaps
              "qboard_bytes_read_per_sample": n * 17 + k * (n // 64) * 16,
              "answered_of_eligible_last_sample": [int(last["answered"].sum()), int(last["eligible"].sum())], "reads": reads}
        out["by_entries"][str(k)] = by
        print(k, json.dumps(by), flush=True)
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
