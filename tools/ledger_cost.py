#!/usr/bin/env python
"""What a sample of the rumour ledger (include/serf_sim_ledger.h) costs, beside a sample of the series and beside the polled
alternative (run on the GPU box).

usage: python tools/ledger_cost.py [--nodes N] [--entries 1,8,64] [--ticks 40] [--rounds 3] [--limit 300] [--out FILE]
       python tools/ledger_cost.py --only ledger|ledger_noreach|series|none|polled [--n-entries 8] [--ticks 40]
                                   one kind of window in this process, for a rocprofv3 --kernel-trace --stats run of its own

The counterpart of tools/roll_cost.py.  The handle is tools/census_cost.py's (1 Mi nodes, kRandomNodes, fan-out 4, SWIM on) under a
steady load of user events — `--events` of them a tick from random nodes (0.25, the benchmark's rate of API operations, by default; 2
fills every queue to SIM_Q and every packet: the worst case), so that queues and packets hold what a sample has to read.  Windows of `ticks` ticks in ONE sim_step ending in a synchronise: no observer, a series behind every tick, a ledger of 1 / 8 /
64 entries behind every tick with the reach pass (EVENT entries: convergence_many_kernel runs) and without it (ALIVE entries: it
does not); the difference to the window without observer is what a sample adds to a tick, end to end.  The polled alternative —
sim_step(1), sim_convergence_many, the dumps of SIM_ARR_QUEUE and SIM_ARR_INBOX, every tick — is timed over `--polled-ticks` ticks.
Every kind of window runs in a child process of its own under a time limit (--limit seconds); the first one that fails or runs
out of time ends the run.  The bytes a ledger sample has to read: per node 32 B of rows, 16 B per four keys plus 16 B per queued
record, one cell per distinct packet page; plus 16 B x nodes per entry of kinds 1-4 for the reach.  Kernel times proper come from
the --only runs under rocprofv3."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def make(n, events, warm):
    """The handle under load: `events` user events a tick from tick 4 on, injected up front for `span` ticks."""
    import numpy as np
    import serf_amd
    from serf_amd import _ffi
    kw = dict(fanout=4, view_slots=1024, event_ring=512, query_ring=512, probe_interval=5, push_pull_interval=150, loss=0.0,
              ring_overflow=8, join_sync=True, flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT)
    sim = serf_amd.create(n, **kw)
    rng = np.random.default_rng(3)
    keys = []
    for t in range(4, 4 + warm["span"]):
        for j in range(int((t + 1) * events) - int(t * events)):   # (a rate below 1: an event every 1 / events ticks)
            key = 0x70000000 + len(keys)
            sim.inject(t, _ffi.OP_USER_EVENT, int(rng.integers(0, n)), key, 64)
            keys.append(key)
    sim.step(warm["ticks"])
    sim.sync()
    return sim, keys


def event_entries(sim, count):
    """`count` EVENT identities that are queued somewhere now, found through the canonical dump of a few thousand nodes' queues
    (the whole dump is a GiB at 1 Mi nodes: what this tool is about)."""
    import numpy as np
    from serf_amd import _ffi
    q = sim.dump(_ffi.ARR_QUEUE)
    q = q[q["meta"] != 0xFFFFFFFF]
    ev = q[((q["meta"] >> 4) & 0xF) == _ffi.K_EVENT]
    ids = sorted({(int(_ffi.K_EVENT), int(k), int(v)) for k, v in zip(ev["key"].tolist(), ev["val"].tolist())})
    out = ids[-count:]
    k = 1
    while len(out) < count:            # (fewer live events than asked for: events nobody sent fill the list)
        out.append((int(_ffi.K_EVENT), 0x7F000000 + k, 1))
        k += 1
    return out


def one(a):
    from census_cost import timed  # noqa: E402  (imports torch first: one HIP runtime per process)
    from serf_amd import _ffi
    warm = dict(span=a.ticks * (a.rounds + 2) + 60, ticks=30)
    sim, keys = make(a.nodes, a.events, warm)
    res = {"nodes": a.nodes, "what": a.only, "entries": a.n_entries, "ticks": a.ticks}
    if a.only == "polled":
        ent = event_entries(sim, a.n_entries)
        t0 = time.perf_counter()
        for _ in range(a.polled_ticks):
            sim.step(1)
            sim.convergence_many(ent)
            sim.dump(_ffi.ARR_QUEUE)
            sim.dump(_ffi.ARR_INBOX)
        res["step_us"] = [(time.perf_counter() - t0) / a.polled_ticks * 1e6]
        res["ticks"] = a.polled_ticks
    else:
        us = []
        for r in range(a.rounds):
            if a.only == "series":
                sim.series_start(0, 1, a.ticks + 4)
            elif a.only == "ledger":
                sim.ledger_start(event_entries(sim, a.n_entries), 0, 1, a.ticks + 4)
            elif a.only == "ledger_noreach":
                sim.ledger_start([(_ffi.K_ALIVE, 7 * i, 0) for i in range(a.n_entries)], 0, 1, a.ticks + 4)
            if a.only != "none":
                sim.step(2)          # first launches
            us.append(timed(sim, a.ticks))
            if a.only == "series":
                assert len(sim.series_read()) == a.ticks + 2
                sim.series_stop()
            elif a.only.startswith("ledger"):
                hdr, rec = sim.ledger_read()
                assert len(hdr) == a.ticks + 2
                res["last_sample"] = {f: int(hdr[f][-1]) for f in hdr.dtype.names}
                res["entries_carried_in_last_sample"] = int(((rec["queued"][-1] + rec["in_flight"][-1]) > 0).sum())
                sim.ledger_stop()
        res["step_us"] = us
    cs = sim.cluster_stats()
    res["overflow"], res["up"] = int(cs["overflow"]), int(cs["up"])
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--entries", default="1,8,64")
    ap.add_argument("--n-entries", type=int, default=8)
    ap.add_argument("--events", type=float, default=0.25, help="user events injected per tick (0.25: the benchmark's rate of API operations; 2 fills every queue to SIM_Q: the worst case)")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--polled-ticks", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds one kind of window may take")
    ap.add_argument("--only", choices=("none", "series", "ledger", "ledger_noreach", "polled"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.only:
        return one(a)
    runs = [("none", 1), ("series", 1)] + [(w, int(k)) for k in a.entries.split(",") for w in ("ledger", "ledger_noreach")] + [("polled", 8)]
    out = {"nodes": a.nodes, "ticks": a.ticks, "events_per_tick": a.events, "windows": []}
    for what, k in runs:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", what, "--n-entries", str(k), "--nodes", str(a.nodes), "--ticks", str(a.ticks),
               "--rounds", str(a.rounds), "--events", str(a.events), "--polled-ticks", str(a.polled_ticks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"{what} {k}: no result within {a.limit} s; stopping", flush=True)
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"{what} {k}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
            break
        res = json.loads(line[-1][7:])
        res["median_us"] = sorted(res["step_us"])[len(res["step_us"]) // 2]
        out["windows"].append(res)
        print(what, k, json.dumps(res), flush=True)
    base = next((w["median_us"] for w in out["windows"] if w["what"] == "none"), None)
    if base is not None:
        for w in out["windows"]:
            w["added_us_per_tick"] = w["median_us"] - base
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
