#!/usr/bin/env python
"""What a sample of the rumour tree (include/serf_sim_tree.h) costs, beside a spread sample of the same entries and a traffic
sample of the same state, for both fan-out models (run on the GPU box).

usage: python tools/tree_cost.py [--nodes N] [--fans krandomnodes,bijection] [--entries 1,16,64] [--ticks 10] [--rounds 3] [--out FILE]
       python tools/tree_cost.py --only tree|spread|traffic|none --fans krandomnodes --entries 16 [--ticks 10]
                                 one kind of window, for a rocprofv3 --kernel-trace --stats run of its own

Four handles of one configuration and one script — `entries` user events from random nodes at tick 0 — go through the same
states: one without an observer, one with a spread map of the events, one with the traffic meter, one with the tree, each
sampling behind every tick.  The same two windows of `ticks` ticks in ONE sim_step ending in a synchronise are timed on each,
the handles taking turns: MID-SPREAD from tick 3 on, while the events travel and carriers are many, and AT REST from tick
`--rest` on, when every node has every event and nothing of them is in flight.  That is repeated `rounds` times on fresh handles;
the differences of the medians against the handle without an observer are what a sample of each adds to a tick, end to end —
the library has no events of its own around an observer's launches, so a sample is timed through the step that carries it — and
spread + traffic is the yardstick: the tree does the work of both plus the match of the records.  The spread of the bare handle's
windows is printed beside them: a difference below it is not measured.  The reads are timed once at the end."""
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

FANS = {"krandomnodes": _ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT, "bijection": _ffi.CF_BASELINE_JOINED}
KINDS = ("none", "spread", "traffic", "tree")
MID_FROM = 3


def median(x):
    return sorted(x)[len(x) // 2]


def make(n, fan, k, kind, capacity):
    """The handle with k user events sent at tick 0 from random nodes and the observer `kind` started before them."""
    kw = dict(fanout=4, view_slots=1024, event_ring=512, query_ring=512, probe_interval=5, push_pull_interval=150, loss=0.0,
              ring_overflow=8, join_sync=True, flags=FANS[fan])
    sim = serf_amd.create(n, **kw)
    rng = np.random.default_rng(3)
    nodes = rng.choice(n, k, replace=False).tolist()
    entries = [(_ffi.K_EVENT, 0x5D000000 + i, int(sim.stats(x).event_time)) for i, x in enumerate(nodes)]
    if kind == "spread":
        sim.spread_start(entries, 0, 1, capacity)
    elif kind == "traffic":
        sim.traffic_start(0, 1, capacity)
    elif kind == "tree":
        sim.tree_start(entries, 0, capacity)
    for i, x in enumerate(nodes):
        sim.user_event(x, 0x5D000000 + i, 64)
    return sim


def timed_call(sim, fn):
    sim.sync()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--fans", default="krandomnodes,bijection")
    ap.add_argument("--entries", default="1,16,64")
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--rest", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.nodes
    cap = a.rest + a.ticks + 4
    out = {"nodes": n, "ticks": a.ticks, "mid_from": MID_FROM, "rest_from": a.rest, "rounds": a.rounds, "runs": []}
    for fan in a.fans.split(","):
        for k in (int(x) for x in a.entries.split(",")):
            if a.only:
                sim = make(n, fan, k, a.only, cap)
                sim.step(MID_FROM)
                mid = timed(sim, a.ticks)
                sim.step(a.rest - int(sim.tick))
                print(json.dumps({"nodes": n, "fanout": fan, "entries": k, "only": a.only, "mid_us": mid, "rest_us": timed(sim, a.ticks)}))
                sim.close()
                continue
            mid, rest = {kd: [] for kd in KINDS}, {kd: [] for kd in KINDS}
            last = reads = None
            for r in range(a.rounds):
                sims = {kd: make(n, fan, k, kd, cap) for kd in KINDS}
                for s in sims.values():
                    s.step(MID_FROM)          # first launches of every kernel
                for kd, s in sims.items():    # the handles take turns: what shares the machine meets all of them
                    mid[kd].append(timed(s, a.ticks))
                for s in sims.values():
                    s.step(a.rest - int(s.tick))
                for kd, s in sims.items():
                    rest[kd].append(timed(s, a.ticks))
                assert len({s.digest() for s in sims.values()}) == 1, "the four handles went through the same states"
                t = sims["tree"]
                hdr, rec = t.tree_read()
                assert len(hdr) == a.rest + a.ticks
                last = {"mid": {f: int(rec[f][MID_FROM + a.ticks - 1].sum()) for f in ("new", "reached", "copies", "fresh")},
                        "rest": {f: int(rec[f][-1].sum()) for f in ("new", "reached", "copies", "fresh")}}
                if r + 1 == a.rounds:
                    s0 = t.tree_summary()[0]
                    reads = {"links_all_us": timed_call(t, lambda: t.tree_links(0)), "links_16_us": timed_call(t, lambda: t.tree_links(0, 0, 16)),
                             "summary_us": timed_call(t, t.tree_summary), "top10_us": timed_call(t, lambda: t.tree_top(0, 10)),
                             "top64_us": timed_call(t, lambda: t.tree_top(0, 64)), "path_us": timed_call(t, lambda: t.tree_path(0, n - 1)),
                             "entry0": {f: int(s0[f]) for f in ("reached", "orphans", "depth", "hop_sum", "most_children")},
                             "entry0_hop_bins": [int(x) for x in s0["hop_bins"]]}
                for s in sims.values():
                    s.close()
            run = {"fanout": fan, "entries": k, "reads": reads, "state": last}
            for name, w in (("mid", mid), ("rest", rest)):
                base = median(w["none"])
                add = {kd: median(w[kd]) - base for kd in KINDS[1:]}
                yard = add["spread"] + add["traffic"]
                run[name] = {"step_us": w, "none_spread_us": max(w["none"]) - min(w["none"]),
                             "added_us_per_sample": add, "spread_plus_traffic_us": yard, "tree_over_yardstick": add["tree"] / yard if yard > 0 else None}
            out["runs"].append(run)
            print(json.dumps(run), flush=True)
    if not a.only:
        if a.out:
            json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
