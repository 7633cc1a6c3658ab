#!/usr/bin/env python
"""What a sample of the member gazette (include/serf_sim_gazette.h) costs beside a census and a roll (run on the GPU box).

usage: python tools/gazette_cost.py [--nodes N] [--view-slots 1024] [--slots 16,64] [--ticks 40] [--rounds 3] [--out FILE]
       python tools/gazette_cost.py --only 64 [--ticks 40]      one sampled window, for a rocprofv3 --kernel-trace --stats run of its own

tools/census_cost.py's set-up: one handle of N nodes with the SWIM layer on, kRandomNodes fan-out and no packet loss.  For every
slot count K of --slots, members leave until K view slots are in use; then windows of `ticks` ticks in ONE sim_step ending in a
synchronise go round — no observer, a census, a roll, a gazette, each behind every tick, on the same handle — `rounds` times.  The
difference of the medians is what a sample adds to a tick, end to end.  By bytes a gazette sample reads what the census's count
kernel reads (the 16-byte heads' lines: 16 B x K x N) plus 4 B x K x N of shadow and writes almost nothing, so the census's added
microseconds from the same run are the yardstick: `ratio_to_census`; `ratio_to_roll` likewise."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime per process: torch's first)

import serf_amd  # noqa: E402
from serf_amd import _ffi  # noqa: E402


def timed(sim, ticks):
    sim.sync()
    t0 = time.perf_counter()
    sim.step(ticks)
    sim.sync()
    return (time.perf_counter() - t0) / ticks * 1e6


def grow(sim, k, nxt):
    """Members leave until k view slots are in use; returns the next node to use."""
    while int(sim.cluster_stats()["slots_in_use"]) < k:
        sim.leave(nxt)
        nxt += 7
    sim.step(2)
    sim.sync()
    return nxt


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--view-slots", type=int, default=1024)
    ap.add_argument("--slots", default="16,64")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.nodes
    kw = dict(fanout=4, view_slots=a.view_slots, event_ring=512, query_ring=512, probe_interval=5, push_pull_interval=150, loss=0.0,
              ring_overflow=8, join_sync=True, flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT)
    sim = serf_amd.create(n, **kw)
    sim.step(4)
    nxt = 3
    cap = a.ticks + 4
    observers = {"census": (lambda: sim.census_start(0, 1, cap, 64), sim.census_stop),
                 "roll": (lambda: sim.roll_start(0, 1, cap, 8), sim.roll_stop),
                 "gazette": (lambda: sim.gazette_start(0, 1, cap, 60), sim.gazette_stop)}
    if a.only is not None:
        nxt = grow(sim, a.only, nxt)
        sim.gazette_start(0, 1, cap, 60)
        sim.step(2)
        us = timed(sim, a.ticks)
        s = sim.gazette_read()
        print(json.dumps({"nodes": n, "slots": int(s["slots"][-1]), "step_us": us, "samples": len(s), "bytes_per_sample": 20 * int(s["slots"][-1]) * n}))
        return
    out = {"nodes": n, "view_slots": a.view_slots, "ticks": a.ticks, "by_slots": {}}
    for k in [int(x) for x in a.slots.split(",")]:
        nxt = grow(sim, k, nxt)
        timed(sim, 10)
        us = {"none": [], "census": [], "roll": [], "gazette": []}
        for r in range(a.rounds):
            us["none"].append(timed(sim, a.ticks))
            for name, (start, stop) in observers.items():
                start()
                sim.step(2)          # first launches (the gazette: its shadow's groups)
                us[name].append(timed(sim, a.ticks))
                if name == "gazette":
                    s = sim.gazette_read()
                    assert len(s) == a.ticks + 2 and int(s["slots"][-1]) >= k
                    k = int(s["slots"][-1])          # (what the samples really covered)
                stop()
        med = {name: median(v) for name, v in us.items()}
        added = {name: med[name] - med["none"] for name in observers}
        out["by_slots"][str(k)] = {"step_us": us, "median_us": med, "range_us": {name: [min(v), max(v)] for name, v in us.items()},
                                   "added_us_per_sample": added, "bytes_per_sample": 20 * k * n,
                                   "ratio_to_census": added["gazette"] / max(added["census"], 1e-9),
                                   "ratio_to_roll": added["gazette"] / max(added["roll"], 1e-9)}
        print(k, json.dumps(out["by_slots"][str(k)]), flush=True)
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
