#!/usr/bin/env python
"""What a sample of the detection log (include/serf_sim_detect.h) costs beside a sample of the census (run on the GPU box).

usage: python tools/detect_cost.py [--nodes N] [--view-slots 1024] [--slots 64,1024] [--ticks 40] [--rounds 5] [--out FILE]
       python tools/detect_cost.py --only 1024 [--ticks 40]     one sampled window, for a rocprofv3 --kernel-trace --stats run of its own

The handle of tools/census_cost.py: N nodes with the SWIM layer on, kRandomNodes fan-out and no packet loss.  For every slot
count K of --slots, members leave until K view slots are in use; then windows of `ticks` ticks in ONE sim_step ending in a
synchronise — once the leaves have been digested and two windows in a row take the same time — alternate between no observer, a census behind every tick and a detection log behind every tick, `rounds` times.
The differences of the medians are what a sample of each adds to a tick, end to end.  A detection sample is the census's count and
fold kernels plus detect_kernel where the census has its pack kernel: the two figures are expected to be equal within the spread
of the census's own alternations (the spread is printed).  detect_kernel's time alone comes from the --only run under rocprofv3."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from census_cost import grow, timed  # noqa: E402  (imports torch first: one HIP runtime per process)

import serf_amd  # noqa: E402
from serf_amd import _ffi  # noqa: E402


def median(x):
    return sorted(x)[len(x) // 2]


def settle(sim, ticks, tries=60):
    """The leaves that took the slots are rumours the cluster has to digest first (queues, suspicion of the members that stop):
    windows without an observer until two in a row take the same time within 2 %."""
    last = timed(sim, ticks)
    for _ in range(tries):
        now = timed(sim, ticks)
        if abs(now - last) <= 0.02 * last:
            return
        last = now


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--view-slots", type=int, default=1024)
    ap.add_argument("--slots", default="64,1024")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.nodes
    kw = dict(fanout=4, view_slots=a.view_slots, event_ring=512, query_ring=512, probe_interval=5, push_pull_interval=150, loss=0.0,
              ring_overflow=8, join_sync=True, flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT)
    sim = serf_amd.create(n, **kw)
    sim.step(4)
    nxt = 3
    if a.only is not None:
        nxt = grow(sim, a.only, nxt)
        sim.detect_start(0, 1, a.ticks + 4, 1 << 16)
        sim.step(2)
        us = timed(sim, a.ticks)
        hdr = sim.detect_read()
        print(json.dumps({"nodes": n, "slots": int(hdr["subjects"][-1]), "step_us": us, "samples": len(hdr),
                          "open_down": int(hdr["open_down"][-1]), "log": sim.detect_log_count()}))
        return
    out = {"nodes": n, "view_slots": a.view_slots, "ticks": a.ticks, "by_slots": {}}
    for k in [int(x) for x in a.slots.split(",")]:
        nxt = grow(sim, k, nxt)
        settle(sim, a.ticks)
        none, cen, det = [], [], []
        for r in range(a.rounds):
            none.append(timed(sim, a.ticks))
            sim.census_start(0, 1, a.ticks + 4, 64)
            sim.step(2)          # first launches
            cen.append(timed(sim, a.ticks))
            sim.census_stop()
            sim.detect_start(0, 1, a.ticks + 4, 1 << 16)
            sim.step(2)
            det.append(timed(sim, a.ticks))
            hdr = sim.detect_read()
            assert len(hdr) == a.ticks + 2 and int(hdr["subjects"][-1]) >= k
            k = int(hdr["subjects"][-1])          # (what the samples really covered)
            sim.detect_stop()
        mn, mc, md = median(none), median(cen), median(det)
        out["by_slots"][str(k)] = {"step_us_none": none, "step_us_census": cen, "step_us_detect": det,
                                   "census_added_us_per_sample": mc - mn, "detect_added_us_per_sample": md - mn,
                                   "detect_minus_census_us": md - mc, "census_spread_us": max(cen) - min(cen),
                                   "detect_spread_us": max(det) - min(det), "none_spread_us": max(none) - min(none)}
        print(k, json.dumps(out["by_slots"][str(k)]), flush=True)
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
