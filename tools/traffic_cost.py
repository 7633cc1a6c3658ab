#!/usr/bin/env python
"""What a sample of the traffic meter (include/serf_sim_traffic.h) costs, beside a series sample and a ledger sample on the same
handle, for both fan-out models (run on the GPU box).

usage: python tools/traffic_cost.py [--nodes N] [--fans krandomnodes,bijection] [--ticks 40] [--rounds 3] [--ledger-entries 16] [--out FILE]
       python tools/traffic_cost.py --only traffic|series|ledger|none --fans krandomnodes [--ticks 40]
                                    one kind of window, for a rocprofv3 --kernel-trace --stats run of its own

The handle is tools/census_cost.py's (1 Mi nodes, fan-out 4, SWIM on) under SIM_CF_RANDOM_FANOUT or the bijection, with user
events injected up front, `--events` a tick from random nodes for as long as the windows run: every node has records queued and
sends its four packets in every tick, so a sample sees a full inbox.  Windows of `ticks` ticks in ONE sim_step ending in a
synchronise alternate between no observer, the series, a ledger of the first `--ledger-entries` events and the traffic meter,
each behind every tick, `rounds` times; the differences of the medians are what a sample of each adds to a tick, end to end.

Bytes a node by the meter's own count, from the samples of the last window (d = packets addressed to a node, the mean over the
nodes; s = the share of nodes that sent): the send pass reads the map word (4 B) and 16 B of every page of every distinct packet,
writes the 8-byte summary and reads and writes 3 x 4 B of the tx columns of a sender; the receive pass reads 4 B of the row
index, per packet 4 B of the row and 8 B of the sender's summary — a scattered read, a 64-byte line fetched for 8 B used — 16 B of
the node's row, and reads and writes the rx columns (3 x 4 B, the peak, rx_down where it does not run).  Printed as "requested" and, with
every gather counted as a whole line, "fetched".  The reads of the map are timed once at the end."""
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
LINE = 64


def median(x):
    return sorted(x)[len(x) // 2]


def make(n, fan, events, ticks, k):
    """The handle with `events` user events a tick from random nodes until tick `ticks`: the first k sent one tick at a time, so that
    each one's Lamport time is read off its origin (they are the ledger's entries), the rest injected up front."""
    kw = dict(fanout=4, view_slots=1024, event_ring=512, query_ring=512, probe_interval=5, push_pull_interval=150, loss=0.0,
              ring_overflow=8, join_sync=True, flags=FANS[fan])
    sim = serf_amd.create(n, **kw)
    rng = np.random.default_rng(3)
    entries, sent = [], 0
    while len(entries) < k:
        for node in rng.choice(n, events, replace=False).tolist():
            entries.append((_ffi.K_EVENT, 0x5C000000 + sent, int(sim.stats(node).event_time)))
            sim.user_event(node, 0x5C000000 + sent, 64)
            sent += 1
        sim.step(1)
    for t in range(int(sim.tick), ticks):
        for node in rng.choice(n, events, replace=False).tolist():
            sim.inject(t, _ffi.OP_USER_EVENT, node, 0x5C000000 + sent, 64)
            sent += 1
    return sim, entries[:k]


def timed_call(sim, fn):
    sim.sync()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def bytes_per_node(samples, n, pages):
    s = samples[-1]
    d = float(s["packets"]) / n
    sent = float(s["senders"]) / n
    addressed = float(s["addressed"]) / n
    send = 4 + 16 * pages * sent + 8 + 24 * sent
    recv_req = 4 + d * (4 + 8) + 16 + addressed * (24 + 8)
    recv_fetch = 4 + d * (4 + LINE) + 16 + addressed * (24 + 8)
    return {"packets_per_node": d, "senders_share": sent, "requested": send + recv_req, "fetched_with_whole_lines": send + recv_fetch,
            "of_that_gathers_requested": d * 8, "of_that_gathers_fetched": d * LINE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--fans", default="krandomnodes,bijection")
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--events", type=int, default=2)
    ap.add_argument("--ledger-entries", type=int, default=16)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.nodes
    out = {"nodes": n, "ticks": a.ticks, "by_fanout": {}}
    for fan in a.fans.split(","):
        windows = 1 if a.only else 4 * a.rounds
        warm = 16
        sim, es = make(n, fan, a.events, warm + windows * (a.ticks + 4) + 8, a.ledger_entries)
        sim.step(max(0, warm - int(sim.tick)))   # the first events have reached everybody: every node sends
        if a.only:
            if a.only == "traffic":
                sim.traffic_start(0, 1, a.ticks + 4)
            elif a.only == "series":
                sim.series_start(0, 1, a.ticks + 4)
            elif a.only == "ledger":
                sim.ledger_start(es, 0, 1, a.ticks + 4)
            sim.step(2)
            print(json.dumps({"nodes": n, "fanout": fan, "only": a.only, "step_us": timed(sim, a.ticks)}))
            sim.close()
            continue
        none, ser, led, trf = [], [], [], []
        samples = None
        for r in range(a.rounds):
            sim.step(2)
            none.append(timed(sim, a.ticks))
            sim.series_start(0, 1, a.ticks + 4)
            sim.step(2)                  # first launches
            ser.append(timed(sim, a.ticks))
            sim.series_stop()
            sim.ledger_start(es, 0, 1, a.ticks + 4)
            sim.step(2)
            led.append(timed(sim, a.ticks))
            sim.ledger_stop()
            sim.traffic_start(0, 1, a.ticks + 4)
            sim.step(2)
            trf.append(timed(sim, a.ticks))
            samples = sim.traffic_read()
            assert len(samples) == a.ticks + 2
            if r + 1 < a.rounds:
                sim.traffic_stop()
        mn, ms, ml, mt = median(none), median(ser), median(led), median(trf)
        reads = {"nodes_all_us": timed_call(sim, lambda: sim.traffic_nodes()), "nodes_16_us": timed_call(sim, lambda: sim.traffic_nodes(0, 16)),
                 "top10_us": timed_call(sim, lambda: sim.traffic_top(10, 5)), "top64_us": timed_call(sim, lambda: sim.traffic_top(64, 5)),
                 "summary_us": timed_call(sim, lambda: sim.traffic_summary(5, 16))}
        rates = _ffi.traffic_rates(sim.traffic_nodes(), len(samples))
        last = samples[-1]
        by = {"step_us_none": none, "step_us_series": ser, "step_us_ledger": led, "step_us_traffic": trf,
              "series_added_us_per_sample": ms - mn, "ledger_added_us_per_sample": ml - mn, "traffic_added_us_per_sample": mt - mn,
              "none_spread_us": max(none) - min(none), "ledger_entries": len(es),
              "bytes_per_node": bytes_per_node(samples, n, 1),
              "last_sample": {k: int(last[k]) for k in ("tick", "running", "packets", "records", "units", "senders", "addressed", "to_down",
                                                        "max_packets", "max_units", "packet_records_max", "packet_units_max")},
              "degree_bins": [int(x) for x in last["degree_bins"]],
              "rx_bytes_per_s": rates["rx_stats"], "tx_bytes_per_s": rates["tx_stats"], "reads": reads}
        out["by_fanout"][fan] = by
        print(fan, json.dumps(by), flush=True)
        sim.traffic_stop()
        sim.close()
    if not a.only:
        print(json.dumps(out))
        if a.out:
            json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
