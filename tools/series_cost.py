#!/usr/bin/env python
"""What a device-resident time series costs, on the benchmark workload (run on the GPU box).

usage: python tools/series_cost.py [--nodes N] [--ticks 120] [--rounds 3] [--periods 1,10,100] [--rate R --pkt-records P --ring-overflow X]
                                   [--only-period P] [--skip-poll] [--out FILE]

1. Cost of sampling: bench.py's configuration and schedule (headline fan-out model, untimed pre-roll into the stationary
   load; --rate / --pkt-records / --ring-overflow move it into the loaded regime with deep queues), then `ticks` ticks in
   ONE sim_step ending in a synchronise, with no series and with a series of period 1 / 10 / 100.  The configurations
   alternate `rounds` times, every round on a handle of its own (the schedule is finite).  Bytes the sample kernel has to
   read at least, computed from the state at the end of a window by the same rule the kernel follows: four 16-byte row
   groups a node, the map word of the node's packets (4 B; with random fan-out it sits in a 64-byte cell of its own
   line), 16 B per group of four queue keys a running node's count says are in use, 8 B of slot mask per deep node,
   32 B of timers where a deadline is set, 16 B of record heads per page of every distinct packet.
2. Against the only alternative: `sim_step(1)` + `sim_cluster_stats_get` per tick (synchronises, hipMalloc / hipFree per
   call, sums over stopped processes too, no histograms) against `sim_step(n)` with a series of period 1 and one
   `sim_series_read`; wall time per tick.
`--only-period P`: just a sampled window of period P (0: none) for a rocprofv3 --kernel-trace --stats run of its own.
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


def timed(sim, ticks):
    sim.sync()
    t0 = time.perf_counter()
    sim.step(ticks)
    sim.sync()
    return (time.perf_counter() - t0) / ticks * 1e6


def bytes_to_read(sim, random_fanout):
    """The least one launch of series_sample_kernel has to read of the state `sim` is in (see above)."""
    import numpy as np
    rows = sim.dump(_ffi.ARR_ROWS)
    n = len(rows)
    up = (rows["flags"] & 1).astype(bool)
    meta = sim.dump(_ffi.ARR_QUEUE)["meta"].reshape(n, -1)
    depth = (meta != 0xFFFFFFFF).sum(axis=1)[up]
    hm = sim.dump(_ffi.ARR_INBOX)["hi_meta"].reshape(-1, n, 4)
    pages = int(((hm >> 4) & 0xF != 0).any(axis=2).sum())   # pages with a record, once per SLOT: an upper bound of the distinct ones
    return {"rows": 64 * n, "map_words": (64 if random_fanout else 4) * n, "queue_keys": int(16 * ((depth + 3) // 4).sum()),
            "deep_masks": int(8 * (depth > 16).sum()), "timers": int(32 * (rows["susp_next"][up] != 0).sum()),
            "packet_heads_at_most": 16 * pages, "deepest_queue": int(depth.max()), "deep_nodes": int((depth > 16).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--ticks", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--periods", default="1,10,100")
    ap.add_argument("--only-period", type=int, default=None)
    ap.add_argument("--skip-poll", action="store_true")
    ap.add_argument("--fanout-model", default="krandomnodes", choices=["bijection", "krandomnodes"])
    ap.add_argument("--rate", type=float, default=None, help="API operations per tick (default: the bench's)")
    ap.add_argument("--pkt-records", type=int, default=None)
    ap.add_argument("--ring-overflow", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    extra = []
    for flag, v in (("--rate", a.rate), ("--pkt-records", a.pkt_records), ("--ring-overflow", a.ring_overflow)):
        if v is not None:
            extra += [flag, str(v)]
    args = bench.parse_args(["--nodes-per-gpu", str(a.nodes), "--fanout-model", a.fanout_model] + extra)
    n = a.nodes
    kw, ops = bench.workload(args, n)
    periods = [int(x) for x in a.periods.split(",")]
    configs = [0] + periods
    assert args.preroll + 24 + max(len(configs) * (a.ticks + 2), 2 * a.ticks) <= bench.horizon(args), "the timed ticks must lie inside the workload's schedule"

    def fresh():   # a handle in the stationary load (the schedule ends at bench.horizon: every round gets its own)
        sim = serf_amd.create(n, **kw)
        for o in ops:
            sim.inject(*o)
        sim.step(args.preroll)
        sim.sync()
        return sim

    def window(sim, period):
        if period:
            sim.series_start(0, period, a.ticks + 8)
            sim.step(2)   # first launches of the two kernels
        us = timed(sim, a.ticks)
        if period:
            taken, dropped = sim.series_count()
            rec = sim.series_read()
            assert dropped == 0 and len(rec) == taken and abs(taken - (a.ticks + 2) / period) <= 1 and int(rec["tick"][-1]) <= sim.tick
            sim.series_stop()
        return us

    sim = fresh()
    if a.only_period is not None:
        us = window(sim, a.only_period)
        print(json.dumps({"nodes": n, "period": a.only_period, "step_us": us, "bytes_at_least": bytes_to_read(sim, a.fanout_model == "krandomnodes")}))
        return
    res = {p: [] for p in configs}
    for r in range(a.rounds):
        if r:
            sim.close()
            sim = fresh()
        timed(sim, 20)   # warm
        for p in (configs if r % 2 == 0 else configs[::-1]):
            us = window(sim, p)
            res[p].append(us)
            print(f"round {r} period {p or 'none'}: step {us:.1f} us", flush=True)
    med = {p: sorted(v)[len(v) // 2] for p, v in res.items()}
    by = bytes_to_read(sim, a.fanout_model == "krandomnodes")
    out = {"nodes": n, "fanout_model": a.fanout_model, "ticks": a.ticks, "workload": extra,
           "step_us_median": {str(p or "none"): med[p] for p in configs}, "step_us_all": {str(p or "none"): res[p] for p in configs},
           "added_us_per_sample": {str(p): (med[p] - med[0]) * p for p in periods},
           "sample_kernel_bytes_at_least": by, "sample_kernel_bytes_sum": sum(v for k, v in by.items() if k not in ("deepest_queue", "deep_nodes")),
           "model_bound_drops": int(sim.cluster_stats()["overflow"])}
    if not a.skip_poll:   # 2. against a poll per tick
        poll, ser = [], []
        for r in range(a.rounds):
            sim.close()
            sim = fresh()
            t0 = time.perf_counter()
            for _ in range(a.ticks):
                sim.step(1)
                sim.cluster_stats()       # synchronises
            poll.append((time.perf_counter() - t0) / a.ticks * 1e6)
            sim.series_start(0, 1, a.ticks)
            sim.sync()
            t0 = time.perf_counter()
            sim.step(a.ticks)
            rec = sim.series_read()       # synchronises
            ser.append((time.perf_counter() - t0) / a.ticks * 1e6)
            assert len(rec) == a.ticks
            sim.series_stop()
            print(f"round {r}: poll per tick {poll[-1]:.1f} us/tick, series {ser[-1]:.1f} us/tick", flush=True)
        mp, ms = sorted(poll)[len(poll) // 2], sorted(ser)[len(ser) // 2]
        out["against_poll"] = {"poll_us_per_tick": poll, "series_us_per_tick": ser, "ratio_of_medians": mp / ms}
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
