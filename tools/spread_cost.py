#!/usr/bin/env python
"""What a sample of the spread map (include/serf_sim_spread.h) costs, beside a ledger sample of the same entries on the same
state and beside the polled alternative (run on the GPU box).

usage: python tools/spread_cost.py [--nodes N] [--entries 1,16,64] [--ticks 40] [--rounds 3] [--polled-ticks 4] [--polled-nodes 65536] [--out FILE]
       python tools/spread_cost.py --only spread|ledger|none [--n-entries 16] [--ticks 40]
                                   one kind of window, for a rocprofv3 --kernel-trace --stats run of its own

The handle is tools/census_cost.py's (1 Mi nodes, kRandomNodes, fan-out 4, SWIM on) with user events sent two a tick from random
nodes for the first `--entries` ticks, so that every entry is a rumour that travels while the windows run.  Windows of `ticks`
ticks in ONE sim_step ending in a synchronise alternate between no observer, a ledger of the entries behind every tick and a
spread map of the same entries behind every tick, `rounds` times; the differences of the medians are what a sample of each adds
to a tick, end to end.  The latch pass reads what the ledger's reach pass reads — per node and entry a 16-byte ring bucket head
(a second one where the head pair is full), 16 B of the node's row once — plus 4 B per node and entry of the map, and writes 4 B
where it latches; the ledger reads the queues and the packets in flight on top of its reach pass.  The bytes by that count are
printed next to the times.  The polled alternative — sim_step(1), a synchronise, the dumps of SIM_ARR_ERING and SIM_ARR_ROWS —
is timed over `--polled-ticks` ticks on a handle of `--polled-nodes` nodes, for scale (its bytes grow with the nodes).  The reads of the map (summary, unreached, late with every node's record) are
timed once at the end."""
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


def median(x):
    return sorted(x)[len(x) // 2]


def make(n, n_events):
    """The handle and n_events EVENT entries: two events a tick from random nodes, sent one tick at a time so that each entry's
    Lamport time is read off its origin."""
    kw = dict(fanout=4, view_slots=1024, event_ring=512, query_ring=512, probe_interval=5, push_pull_interval=150, loss=0.0,
              ring_overflow=8, join_sync=True, flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT)
    sim = serf_amd.create(n, **kw)
    rng = np.random.default_rng(3)
    entries = []
    while len(entries) < n_events:
        for node in rng.choice(n, 2, replace=False).tolist():
            if len(entries) < n_events:
                key = 0x5B000000 + len(entries)
                entries.append((_ffi.K_EVENT, key, int(sim.stats(node).event_time)))
                sim.user_event(node, key, 64)
        sim.step(1)
    return sim, entries


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
    ap.add_argument("--polled-ticks", type=int, default=4)
    ap.add_argument("--polled-nodes", type=int, default=1 << 16)
    ap.add_argument("--only", default=None)
    ap.add_argument("--n-entries", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.nodes
    counts = [a.n_entries] if a.only else [int(x) for x in a.entries.split(",")]
    sim, entries = make(n, max(counts))
    sim.step(4)
    if a.only:
        es = entries[:a.n_entries]
        if a.only == "spread":
            sim.spread_start(es, 0, 1, a.ticks + 4)
        elif a.only == "ledger":
            sim.ledger_start(es, 0, 1, a.ticks + 4)
        sim.step(2)
        print(json.dumps({"nodes": n, "only": a.only, "entries": len(es), "step_us": timed(sim, a.ticks)}))
        return
    out = {"nodes": n, "ticks": a.ticks, "by_entries": {}}
    for k in counts:
        es = entries[:k]
        none, led, spr = [], [], []
        latched = 0
        for r in range(a.rounds):
            none.append(timed(sim, a.ticks))
            sim.ledger_start(es, 0, 1, a.ticks + 4)
            sim.step(2)          # first launches
            led.append(timed(sim, a.ticks))
            sim.ledger_stop()
            sim.spread_start(es, 0, 1, a.ticks + 4)
            sim.step(2)
            spr.append(timed(sim, a.ticks))
            hdr, rec = sim.spread_read()
            assert len(hdr) == a.ticks + 2
            latched = int(hdr["new"][2:].sum())
            if r + 1 < a.rounds:
                sim.spread_stop()
        mn, ml, ms = median(none), median(led), median(spr)
        reads = {"summary_us": timed_call(sim, lambda: sim.spread_summary(1)), "unreached_us": timed_call(sim, lambda: sim.spread_unreached(0, 64)),
                 "late_top64_us": timed_call(sim, lambda: sim.spread_late(64)), "late_nodes_us": timed_call(sim, lambda: sim.spread_late(64, nodes=True)),
                 "map_us": timed_call(sim, lambda: sim.spread_map(0))}
        sim.spread_stop()
        by = {"step_us_none": none, "step_us_ledger": led, "step_us_spread": spr, "ledger_added_us_per_sample": ml - mn,
              "spread_added_us_per_sample": ms - mn, "spread_minus_ledger_us": ms - ml, "none_spread_us": max(none) - min(none),
              # per sample: 16 B of every node's row, per entry 16 B of a bucket head and 4 B of the map; 4 B written per latch
              "spread_bytes_read_per_sample": n * (16 + k * (16 + 4)), "reach_bytes_read_per_sample": n * (16 + k * 16),
              "spread_bytes_written_last_window": 4 * latched, "reads": reads}
        out["by_entries"][str(k)] = by
        print(k, json.dumps(by), flush=True)
    # the polled alternative: a tick, a synchronise, the ring and the rows over PCIe — on a handle of its own of --polled-nodes nodes
    # (the ring dump is (ring_overflow + event_ring) x nodes x 32 B: 17 GB a tick at 1 Mi nodes); it grows with the nodes
    sim.close()
    sim, _ = make(a.polled_nodes, 2)
    sim.step(4)
    sim.sync()
    t0 = time.perf_counter()
    nbytes = 0
    for _ in range(a.polled_ticks):
        sim.step(1)
        sim.sync()
        nbytes = sim.dump(_ffi.ARR_ERING).nbytes + sim.dump(_ffi.ARR_ROWS).nbytes
    out["polled"] = {"nodes": a.polled_nodes, "us_per_tick": (time.perf_counter() - t0) / a.polled_ticks * 1e6, "bytes_per_tick": nbytes}
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
