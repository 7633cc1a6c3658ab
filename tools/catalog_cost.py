#!/usr/bin/env python
"""What a sample of the rumour catalogue (include/serf_sim_catalog.h) costs, beside a ledger sample of 64 entries on the same
handle (run on the GPU box).

usage: python tools/catalog_cost.py [--nodes N] [--load headline|second] [--ticks 40] [--rounds 3] [--out FILE]
       python tools/catalog_cost.py --only catalog|ledger|none [--load ...] [--ticks 40]
                                    one kind of window, for a rocprofv3 --kernel-trace --stats run of its own

The handle is the benchmark's: bench.workload at 1 Mi nodes, kRandomNodes — `headline` its default load (0.25 API operations a
tick, 4 records a packet), `second` its second_load (--second-rate operations a tick, 16 records a packet, 8 overflow rows) —
rolled through the benchmark's pre-roll into the stationary state.  Windows of `ticks` ticks in ONE sim_step ending in a
synchronise alternate, `rounds` times, between
  none      no observer
  ledger    a ledger of 64 entries behind every tick: the identities sim_catalog_now finds at the window's start (what nobody
            could name before there was a catalogue), filled up with ALIVE entries when there are fewer
  catalog   a catalogue of all kinds behind every tick
and the differences of the medians to `none` are what a sample adds to a tick, end to end; the ranges are printed with them,
and catalog / ledger is the ratio the profile asks for.  The last sample's words say what the scan met: live identities,
queued records, records in flight, overflow."""
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


def spread(x):
    return [min(x), sorted(x)[len(x) // 2], max(x)]


def ledger_entries(sim):
    """64 identities for the ledger: what the catalogue finds now, then ALIVE entries nobody carries."""
    _, live = sim.catalog_now()
    out = [(int(x["id"]) >> 32, int(x["id"]) & 0xFFFFFFFF, int(x["val"])) for x in live[:_ffi.LEDGER_MAX]]
    k = 0
    while len(out) < _ffi.LEDGER_MAX:
        if (_ffi.K_ALIVE, 7 * k, 1 << 30) not in out:
            out.append((_ffi.K_ALIVE, 7 * k, 1 << 30))
        k += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--load", default="headline", choices=["headline", "second"])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["none", "ledger", "catalog"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.nodes
    args = bench.parse_args(["--nodes-per-gpu", str(n), "--fanout-model", "krandomnodes"])
    if a.load == "second":
        args.pkt_records, args.rate, args.preroll, args.ring_overflow = 16, args.second_rate, args.second_preroll, args.second_ring_overflow
    kw, ops = bench.workload(args, n, "krandomnodes")
    kinds = ("none", "ledger", "catalog") if not a.only else (a.only,)
    rounds = a.rounds if not a.only else 1
    assert args.preroll + 24 + rounds * len(kinds) * (a.ticks + 2) <= bench.horizon(args), "the timed ticks must lie inside the workload's schedule"
    sim = serf_amd.create(n, **kw)
    for o in ops:
        sim.inject(*o)
    sim.step(args.preroll)
    timed(sim, 20)   # warm
    res = {k: [] for k in kinds}
    last = None
    for r in range(rounds):
        for kind in (kinds if r % 2 == 0 else kinds[::-1]):
            if kind == "ledger":
                sim.ledger_start(ledger_entries(sim), 0, 1, a.ticks + 4)
            elif kind == "catalog":
                sim.catalog_start(_ffi.CATALOG_KINDS, _ffi.CATALOG_MAX, 0, 1, a.ticks + 4)
            if kind != "none":
                sim.step(2)   # first launches
            us = timed(sim, a.ticks)
            res[kind].append(us)
            if kind == "ledger":
                hdr, rec = sim.ledger_read()
                assert len(hdr) == a.ticks + 2
                carried = int(((rec["queued"][-1] + rec["in_flight"][-1]) > 0).sum())
                sim.ledger_stop()
            elif kind == "catalog":
                s = sim.catalog_read()
                assert len(s) == a.ticks + 2
                last = {f: int(s[f][-1]) for f in ("tick", "running", "live", "overflow", "registry", "ids_lost", "queued", "in_flight", "packets")}
                last["live_by_kind"] = s["live_by_kind"][-1].tolist()
                last["overflowed_samples"] = int(s["overflowed"][-1])
                sim.catalog_stop()
            print(f"round {r} {kind}: step {us:.1f} us", flush=True)
    out = {"nodes": n, "load": a.load, "ticks": a.ticks, "rounds": rounds, "step_us": {k: spread(v) for k, v in res.items()},
           "last_catalog_sample": last, "model_bound_drops": int(sim.cluster_stats()["overflow"])}
    if not a.only:
        base = spread(res["none"])[1]
        out["ledger64_added_us_per_sample"] = spread(res["ledger"])[1] - base
        out["catalog_added_us_per_sample"] = spread(res["catalog"])[1] - base
        out["none_spread_us"] = max(res["none"]) - min(res["none"])
        out["ledger_entries_carried_last_sample"] = carried
        if out["ledger64_added_us_per_sample"] > 0:
            out["catalog_over_ledger64"] = out["catalog_added_us_per_sample"] / out["ledger64_added_us_per_sample"]
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
