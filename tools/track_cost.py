#!/usr/bin/env python
"""What a device-resident tracker costs, on the benchmark workload (run on the GPU box).

usage: python tools/track_cost.py [--nodes N] [--ticks 120] [--rounds 3] [--planes 1,8,64] [--per-plane 6] [--only-planes P --kind view|ring]

1. Cost of tracking: bench.py's configuration and schedule (headline fan-out model, untimed pre-roll into the stationary
   load), then `ticks` ticks in ONE sim_step ending in a synchronise, with no tracker and with 1 / 8 / 64 planes followed,
   `per-plane` trackers on each.  Two kinds of plane: `view` — MEMBER trackers on subjects that hold a view slot (16 B a
   node and plane: the case the byte count below describes; the subjects get their slots from a set_tags each before
   the run, and the handle does not recycle slots); `ring` — EVENT trackers on buckets the workload's own events
   use, with keys that exist nowhere: every node whose bucket head is full goes on to the tail plane, the worst case
   (up to 32 B a node and plane, two dependent loads).  No tracker can hit, so nothing retires and every tick evaluates
   all of them.  The configurations alternate `rounds` times, every round on a handle of its own (the schedule is
   finite).  Bytes the count kernel has to read at least: 16 B x nodes per plane + 16 B x nodes (the row group with the
   up flag).
2. Against a poll per tick: 64 rumours outstanding, `sim_step(1)` + `sim_convergence_many` per tick (the only way
   to follow them without trackers) against `sim_step(n)` with 64 trackers and one read at the end; wall time per tick.
`--only-planes P`: just a tracked window with P planes (for a rocprofv3 --kernel-trace --stats run of its own).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime per process: torch's first)

import bench  # noqa: E402
import serf_amd  # noqa: E402
from serf_amd import _ffi  # noqa: E402


def specs_for(kind, planes, per_plane, ring, slotted):
    if kind == "ring":   # bucket b of the event ring: Lamport time b; keys nobody ever used
        return [_ffi.rumour_tracker(_ffi.K_EVENT, 0x7F000000 + p * 64 + k, 1 + (p * 7) % ring) for p in range(planes) for k in range(per_plane)]
    # view planes: subjects that hold a slot; an incarnation nobody has, so that nothing hits
    assert len(slotted) >= planes, f"only {len(slotted)} subjects hold a view slot"
    masks = [(1 << 4, 0), (1 << 3, 0), (1 << 2, 0), (0, 1 << 1), (0, 1 << 2), (1 << 1, 0), (1 << 0, 0), (0, 1 << 3)]
    return [_ffi.member_tracker(int(slotted[p]), *masks[k % len(masks)], min_inc=0xFFFFFFFF) for p in range(planes) for k in range(per_plane)]


def timed(sim, ticks):
    sim.sync()
    t0 = time.perf_counter()
    sim.step(ticks)
    sim.sync()
    return (time.perf_counter() - t0) / ticks * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--ticks", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--planes", default="1,8,64")
    ap.add_argument("--kind", default="view", choices=["view", "ring"], help="--only-planes: which kind of plane")
    ap.add_argument("--per-plane", type=int, default=6)
    ap.add_argument("--only-planes", type=int, default=None)
    ap.add_argument("--fanout-model", default="krandomnodes", choices=["bijection", "krandomnodes"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    args = bench.parse_args(["--nodes-per-gpu", str(a.nodes), "--fanout-model", a.fanout_model])
    n = a.nodes
    kw, ops = bench.workload(args, n)
    planes = [int(x) for x in a.planes.split(",")]
    configs = [("none", 0)] + [(k, p) for k in ("view", "ring") for p in planes]
    assert args.preroll + 24 + max(len(configs) * (a.ticks + 2), 2 * a.ticks) <= bench.horizon(args), "the timed ticks must lie inside the workload's schedule"

    kw["recycle_interval"] = 0   # the followed subjects keep their view slots through the timed window
    followed = [1000 + 37 * x for x in range(max(planes + [a.only_planes or 0]))]

    def fresh():   # a handle in the stationary load (the schedule ends at bench.horizon: every round gets its own)
        sim = serf_amd.create(n, **kw)
        for x in followed:
            sim.set_tags(x, 1)   # an operation about the node itself: it gets a view slot, hence a plane of its own
        for o in ops:
            sim.inject(*o)
        sim.step(args.preroll)
        sim.sync()
        return sim
    sim = fresh()
    ring = args.ring
    import numpy as np

    def slotted_subjects(sim):
        slot = sim.dump(_ffi.ARR_SLOTMAP)
        return np.array([x for x in followed if slot[x] != 0xFFFFFFFF])
    if a.only_planes is not None:
        ids = sim.track_add(specs_for(a.kind, a.only_planes, a.per_plane, ring, slotted_subjects(sim))) if a.only_planes else []
        us = timed(sim, a.ticks)
        print(json.dumps({"nodes": n, "kind": a.kind, "planes": a.only_planes, "trackers": len(ids), "step_us": us,
                          "count_kernel_bytes_per_tick_at_least": 16 * n * (a.only_planes + 1)}))
        return
    res = {f"{k}:{p}": [] for k, p in configs}
    for r in range(a.rounds):
        if r:
            sim.close()
            sim = fresh()
        timed(sim, 20)   # warm
        slotted = slotted_subjects(sim)
        for k, p in (configs if r % 2 == 0 else configs[::-1]):
            ids = sim.track_add(specs_for(k, p, a.per_plane, ring, slotted)) if p else []
            if ids:
                sim.step(2)   # first launches of the two kernels, the list's upload
            us = timed(sim, a.ticks)
            if ids:
                rs = sim.track_read(ids)
                assert all(x.evaluated == a.ticks + 2 and x.state == 1 and x.peak == 0 for x in rs)
                sim.track_remove(ids)
            res[f"{k}:{p}"].append(us)
            print(f"round {r} {k} planes {p} trackers {len(ids)}: step {us:.1f} us", flush=True)
    med = {c: sorted(v)[len(v) // 2] for c, v in res.items()}
    out = {"nodes": n, "fanout_model": a.fanout_model, "ticks": a.ticks, "per_plane": a.per_plane,
           "step_us_median": med, "step_us_all": res,
           "added_us_per_plane": {f"{k}:{p}": (med[f"{k}:{p}"] - med["none:0"]) / p for k, p in configs if p},
           "count_kernel_bytes_per_tick_at_least": {p: 16 * n * (p + 1) for p in planes}}
    # 2. against a poll per tick: 64 rumours (16 Lamport times x 4 keys)
    rum = [(_ffi.K_EVENT, 0x7E000000 + i, 1 + (i // 4) * 5 % ring) for i in range(64)]
    poll, trk = [], []
    for r in range(a.rounds):
        sim.close()
        sim = fresh()
        t0 = time.perf_counter()
        for _ in range(a.ticks):
            sim.step(1)
            sim.convergence_many(rum)     # synchronises
        poll.append((time.perf_counter() - t0) / a.ticks * 1e6)
        ids = sim.track_add([_ffi.rumour_tracker(*x) for x in rum])
        sim.sync()
        t0 = time.perf_counter()
        sim.step(a.ticks)
        rs = sim.track_read(ids)          # synchronises
        trk.append((time.perf_counter() - t0) / a.ticks * 1e6)
        assert all(x.evaluated == a.ticks for x in rs)
        sim.track_remove(ids)
        print(f"round {r} 64 rumours: poll per tick {poll[-1]:.1f} us/tick, trackers {trk[-1]:.1f} us/tick", flush=True)
    mp, mt = sorted(poll)[len(poll) // 2], sorted(trk)[len(trk) // 2]
    out["rumours_64"] = {"poll_us_per_tick": poll, "tracker_us_per_tick": trk, "ratio_of_medians": mp / mt}
    out["model_bound_drops"] = int(sim.cluster_stats()["overflow"])
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
