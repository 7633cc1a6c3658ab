#!/usr/bin/env python
"""What a sample of the membership census (include/serf_sim_census.h) costs (run on the GPU box).

usage: python tools/census_cost.py [--nodes N] [--view-slots 1024] [--slots 16,64,256,1024] [--ticks 40] [--rounds 3] [--out FILE]
       python tools/census_cost.py --only 64 [--ticks 40]      one sampled window, for a rocprofv3 --kernel-trace --stats run of its own

One handle of N nodes with the SWIM layer on, kRandomNodes fan-out and no packet loss (no false suspicion takes a slot).  For every slot count K of --slots, members leave until K
view slots are in use (a leave takes a slot for its subject at once); then windows of `ticks` ticks in ONE sim_step ending in a
synchronise alternate between no census and a census behind every tick, `rounds` times: the difference of the medians is what a
sample adds to a tick, end to end (three launches, the stream's order).  The bytes a sample has to read are 16 B x K x N (the head
plane of every allocated slot); the figure beside it is a device-to-device copy of as many bytes (at most --copy-cap), timed with
device events in the same process — a copy reads AND writes every byte.  Kernel times proper come from the --only run under
rocprofv3."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (one HIP runtime per process: torch's first)

import serf_amd  # noqa: E402
from serf_amd import _ffi  # noqa: E402


def timed(sim, ticks):
    sim.sync()
    t0 = time.perf_counter()
    sim.step(ticks)
    sim.sync()
    return (time.perf_counter() - t0) / ticks * 1e6


def copy_rate(nbytes, reps=10):
    """Device-to-device copy of nbytes: (microseconds, bytes read per second)."""
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    return us, nbytes / (us * 1e-6)


def grow(sim, k, nxt):
    """Members leave until k view slots are in use; returns the next node to use."""
    while int(sim.cluster_stats()["slots_in_use"]) < k:
        sim.leave(nxt)
        nxt += 7
    sim.step(2)
    sim.sync()
    return nxt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--view-slots", type=int, default=1024)
    ap.add_argument("--slots", default="16,64,256,1024")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--copy-cap", type=int, default=4 << 30)
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
        sim.census_start(0, 1, a.ticks + 4, 64)
        sim.step(2)
        us = timed(sim, a.ticks)
        hdr, _ = sim.census_read()
        k = int(hdr["subjects"][-1])
        print(json.dumps({"nodes": n, "slots": k, "step_us": us, "samples": len(hdr), "bytes_per_sample": 16 * k * n}))
        return
    out = {"nodes": n, "view_slots": a.view_slots, "ticks": a.ticks, "by_slots": {}}
    for k in [int(x) for x in a.slots.split(",")]:
        nxt = grow(sim, k, nxt)
        timed(sim, 10)
        none, cen = [], []
        for r in range(a.rounds):
            none.append(timed(sim, a.ticks))
            sim.census_start(0, 1, a.ticks + 4, 64)
            sim.step(2)          # first launches
            cen.append(timed(sim, a.ticks))
            hdr, _ = sim.census_read()
            assert len(hdr) == a.ticks + 2 and int(hdr["subjects"][-1]) >= k and int(hdr["running"][-1]) <= n
            k = int(hdr["subjects"][-1])          # (what the samples really covered)
            sim.census_stop()
        mn, mc = sorted(none)[len(none) // 2], sorted(cen)[len(cen) // 2]
        nbytes = 16 * k * n
        cus, crate = copy_rate(min(nbytes, a.copy_cap))
        out["by_slots"][str(k)] = {"step_us_none": none, "step_us_census": cen, "added_us_per_sample": mc - mn, "bytes_per_sample": nbytes,
                                   "read_GBps_end_to_end": nbytes / max(mc - mn, 1e-9) / 1e3,
                                   "copy_bytes": min(nbytes, a.copy_cap), "copy_us": cus, "copy_read_GBps": crate / 1e9}
        print(k, json.dumps(out["by_slots"][str(k)]), flush=True)
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
