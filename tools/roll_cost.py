#!/usr/bin/env python
"""What a sample of the observer roll (include/serf_sim_roll.h) costs, beside a sample of the census (run on the GPU box).

usage: python tools/roll_cost.py [--nodes N] [--view-slots 1024] [--slots 16,64,1024] [--ticks 40] [--rounds 3] [--top-k 8] [--out FILE]
       python tools/roll_cost.py --only 64 [--what roll|census] [--ticks 40]   one sampled window, for a rocprofv3 --kernel-trace --stats run of its own

The counterpart of tools/census_cost.py, with its handle and its way of taking slots into use: for every slot count K of --slots,
windows of `ticks` ticks in ONE sim_step ending in a synchronise alternate between no observer, a census behind every tick and a
roll behind every tick, `rounds` times; the difference of the medians is what a sample adds to a tick, end to end.  A roll sweeps
the head plane of every allocated slot twice — the census's count kernel for the per-subject references, then roll_count_kernel —
so the bytes a sample has to read are 2 x 16 B x K x N; a census reads them once.  Kernel times proper come from the --only runs
under rocprofv3."""
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


def window(sim, what, ticks, top_k):
    """One window with `what` behind every tick: (microseconds a tick, subjects the last sample covered)."""
    if what == "none":
        return timed(sim, ticks), None
    if what == "census":
        sim.census_start(0, 1, ticks + 4, 64)
    else:
        sim.roll_start(0, 1, ticks + 4, top_k, _ffi.ROLL_BY_STALE)
    sim.step(2)          # first launches
    us = timed(sim, ticks)
    hdr, _ = sim.census_read() if what == "census" else sim.roll_read()
    assert len(hdr) == ticks + 2
    (sim.census_stop if what == "census" else sim.roll_stop)()
    return us, int(hdr["subjects"][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--view-slots", type=int, default=1024)
    ap.add_argument("--slots", default="16,64,1024")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--top-k", type=int, default=8)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--what", choices=("roll", "census"), default="roll")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.nodes
    kw = dict(fanout=4, view_slots=a.view_slots, event_ring=512, query_ring=512, probe_interval=5, push_pull_interval=150, loss=0.0,
              ring_overflow=8, join_sync=True, flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT)
    sim = serf_amd.create(n, **kw)
    sim.step(4)
    nxt = 3
    if a.only is not None:
        grow(sim, a.only, nxt)
        us, k = window(sim, a.what, a.ticks, a.top_k)
        print(json.dumps({"nodes": n, "what": a.what, "slots": k, "step_us": us, "samples": a.ticks + 2,
                          "bytes_per_sample": (2 if a.what == "roll" else 1) * 16 * k * n}))
        return
    out = {"nodes": n, "view_slots": a.view_slots, "ticks": a.ticks, "top_k": a.top_k, "by_slots": {}}
    for k in [int(x) for x in a.slots.split(",")]:
        nxt = grow(sim, k, nxt)
        timed(sim, 10)
        us = {"none": [], "census": [], "roll": []}
        for r in range(a.rounds):
            for what in ("none", "census", "roll"):
                t, covered = window(sim, what, a.ticks, a.top_k)
                us[what].append(t)
                k = covered or k          # (what the samples really covered)
        med = {w: sorted(v)[len(v) // 2] for w, v in us.items()}
        nbytes = 16 * k * n
        out["by_slots"][str(k)] = {"step_us": us, "census_added_us_per_sample": med["census"] - med["none"],
                                   "roll_added_us_per_sample": med["roll"] - med["none"], "head_plane_bytes": nbytes,
                                   "census_read_GBps_end_to_end": nbytes / max(med["census"] - med["none"], 1e-9) / 1e3,
                                   "roll_read_GBps_end_to_end": 2 * nbytes / max(med["roll"] - med["none"], 1e-9) / 1e3}
        print(k, json.dumps(out["by_slots"][str(k)]), flush=True)
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
