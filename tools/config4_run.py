#!/usr/bin/env python
"""BASELINE configs[4] on one GPU: 5 % churn + 1 % packet loss with the failure detector ON, convergence-round histogram.

`--churn-frac` of the nodes crash one after the other (one every `--churn-every` ticks), stay down `--down` ticks — long
enough to be suspected, confirmed and DECLARED FAILED by the SWIM layer (minimum suspicion timeout 120 ticks at 1 Mi
nodes) — and re-join (Serf::join: refuting incarnation + join intent); every gossip packet AND every probe leg is lost with
probability `--loss`.  Probes that fail on live nodes (0.26 per tick at 1 Mi nodes and 1 %) start false suspicions that
are refuted.  `--rumors` user events are injected at regular intervals from random running nodes; for each the number of
gossip rounds until >= 99 % of the running nodes have applied it is recorded.  The run is valid only if no model bound was
hit (`model_bound_drops` == 0).  The pace of the churn is set by the model's per-node capacity: SIM_S = 16 suspicion timers
(a crashed node is a running suspicion at every node for ~125 ticks); the queue holds 64 entries (r6).

`--tracker`: the same kind of run followed by DEVICE-RESIDENT TRACKERS (include/serf_sim_track.h) instead of a host poll per
tick.  Crashes are drawn with a per-tick probability (`--crash-prob`; a draw is skipped while `--crash-cap` crashed nodes are
still inside their suspicion window: what SIM_S = 16 timers per node allow without drops), user events are injected in bursts
WHILE the churn runs (many outstanding at once), and the run advances in one sim_step per stretch between two bursts.  Output:
histograms of the rounds until 50 / 90 / 99 / 100 % of the running nodes have applied an event, of the ticks from a crash to the
first suspicion and to "declared failed by 99 %", and the number of sampled never-crashed nodes that anybody ever suspected.
The run of profiles/r07_config4_tracker.json (zero drops at 2 Mi nodes): --random-fanout --pkt-records 16 --tcp-fallback --nacks
--reconnect-interval 150 --gossip-to-the-dead 150 --rumors 560 --burst 4 --crash-prob 0.1 --crash-cap 12.  Bursts have to lie further
apart than an event needs to reach everybody: origins that have not seen the last burst give the next one the same Lamport time.

`--series PERIOD`: a DEVICE-RESIDENT TIME SERIES (include/serf_sim_series.h) of the same run — one sample of cluster gauges behind
every PERIOD-th tick (queue entries by class, the queue-depth histogram, health scores, suspicion timers, clock spread, the records
in flight by kind), read once at the end and written into the JSON under "series", one list per field.  It changes nothing else
about the run.  The run of profiles/r08_config4_series.json: the r07 tracker run's options with --series 10.

`--census PERIOD`: a MEMBERSHIP CENSUS (include/serf_sim_census.h) of the same run — behind every PERIOD-th tick the views of every
subject that owns a view slot are counted on the device; the headers' curves (subjects, settled subjects, running subjects held
Failed / Suspect-or-Dead and by how many, stopped subjects still held Alive, stopped subjects everybody knows gone) go into the JSON
under "census", one list per field, with the subjects' records of the run's last tick.  Like --series it changes nothing else about
the run and goes with either kind of run.  The run of profiles/r09_config4_census.json: see profiles/r09_census.md.

`--roll PERIOD`: an OBSERVER ROLL (include/serf_sim_roll.h) of the same run — behind every PERIOD-th tick every running node's view is
measured against the per-subject references on the device; the headers' curves (observers that are current, the sums and maxima of
`stale`, `lag` and the three kinds of accusation, the histogram of `stale`) go into the JSON under "roll", one list per field, with
the 16 worst observers by `stale` of every sample and, for the run's last tick, the 64 worst by accusations.  Like --census it
changes nothing else about the run, and the two go together.  The run of profiles/r10_config4_roll.json: see profiles/r10_roll.md.

`--ledger PERIOD` (with --tracker): a RUMOUR LEDGER (include/serf_sim_ledger.h) of the first 64 user events the trackers follow —
behind every PERIOD-th tick their reach, the copies of them that wait in queues and the copies in flight.  A ledger's entries are
fixed for its life and an event's Lamport time is known only when it is injected, so every burst gets a ledger of its own, started
with the burst and read, summarised (_ffi.ledger_summary: first tick, final reach, copies sent, the tick it died at and the reach
then, copies per node reached) and stopped when the next burst comes: a rumour that outlives the stretch between two bursts shows
"died_at": null.  The summaries go into the JSON under "ledger".  See profiles/r11_ledger.md.

`--spread PERIOD` (with --tracker): a SPREAD MAP (include/serf_sim_spread.h) of the first 64 user events the trackers follow, a map
per burst as for --ledger: when each node first had each event.  Per event the JSON gets, under "spread", the first and last arrival,
the reached and the running nodes never reached, the histogram of arrival - first and the arrival percentiles (_ffi.spread_percentiles).

`--detect PERIOD`: a DETECTION LOG (include/serf_sim_detect.h) behind every PERIOD-th tick: every subject with a view slot is
judged on the device — nobody is named in advance — and the run's JSON gets, under "detect", _ffi.detect_summary over every
episode of the run (per kind and outcome the count and the median and 99th percentile of each latency), the last sample's header
(cumulative counters and the three latency histograms) and the log's counts.  Without the flag nothing about the run changes.
The run of profiles/r12_config4_detect.json (--tracker --detect 1): see profiles/r12_detect.md.

`--tree` (with --tracker): a RUMOUR TREE (include/serf_sim_tree.h) of the first 64 user events the trackers follow, a tree per burst
as for --spread, latched behind every tick: who infected whom.  Per event the JSON gets, under "tree", the reached nodes and the
orphans among them, the depth, the hop histogram and percentiles (_ffi.tree_hops) and the ten nodes with the most children.  See
profiles/r15_tree.md.

`--traffic PERIOD`: a TRAFFIC METER (include/serf_sim_traffic.h) behind every PERIOD-th tick: per node the gossip packets, records and
wire bytes it sent and had addressed to it.  The run's JSON gets, under "traffic", the bytes per second sent and addressed per node
(median, 99th percentile, max and the 99th-percentile-to-median ratio; _ffi.traffic_rates), the ten nodes the most bytes were addressed
to, the share of the packets that were addressed to stopped processes, the summed in-degree histogram of the samples and the
summary of rx_units.  Without the flag nothing about the run changes; it goes with either kind of run.  See profiles/r14_traffic.md.

Needs an MI355X.  Writes one JSON (default profiles/r03_config4_churn5_loss1_swim.json; --tracker: profiles/r07_config4_tracker.json;
--series: profiles/r08_config4_series.json; --census: profiles/r09_config4_census.json; --roll: profiles/r10_config4_roll.json; --detect: profiles/r12_config4_detect.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hist(values):
    import numpy as np
    return {int(k): int(v) for k, v in zip(*np.unique(np.asarray(values, dtype=np.int64), return_counts=True))} if len(values) else {}


def series_json(args, sim):
    """The samples of the run's series, one list per field of _ffi.SERIES_DTYPE (vector fields: one list per sample)."""
    taken, dropped = sim.series_count()
    rec = sim.series_read()
    out = {"period": args.series, "samples": int(taken), "dropped": int(dropped),
           "what": "include/serf_sim_series.h: state after the tick `tick` - 1; per-node figures over RUNNING nodes; depth_bins = nodes with "
                   "0, 1, 2-3, 4-7, 8-15, 16-31, 32-63, 64 queue entries; queued / records by class / kind; len64 in 16-byte units"}
    for name in rec.dtype.names:
        if name != "reserved":
            out[name] = rec[name].tolist()
    return out


ROLL_TOP = 16


def roll_json(args, sim):
    """The headers of the run's roll, one list per field of _ffi.ROLL_HEADER_DTYPE, the listed observers of every sample and the
    worst accusers of the state at the end."""
    from serf_amd import _ffi

    def nodes(rec):
        return [{"id": int(r["id"]) & 0xFFFFFFFF, **{f: int(r[f]) for f in rec.dtype.names if f != "id"}} for r in rec]
    taken, dropped = sim.roll_count()
    hdr, rec = sim.roll_read()
    out = {"period": args.roll, "samples": int(taken), "dropped": int(dropped), "top_k": ROLL_TOP, "rank_by": "stale",
           "what": "include/serf_sim_roll.h: state after the tick `tick` - 1; observers = running nodes, subjects = nodes that own a view "
                   "slot; per observer: unknown / behind = subjects it does not know / knows at an older Lamport time or incarnation "
                   "than some observer, stale = their sum, false_failed / suspects = RUNNING subjects it holds Failed / Suspect or Dead, "
                   "stale_alive = STOPPED subjects it holds Alive, lag = the Lamport times it is behind, summed; current = observers "
                   "with stale 0; stale_bins = observers with stale 0, 1, 2-3, 4-7, ..."}
    for name in hdr.dtype.names:
        out[name] = (hdr[name] & 0xFFFFFFFF).tolist() if name == "listed" else hdr[name].tolist()
    out["worst_by_stale"] = [nodes(r[:int(h["listed"]) & 0xFFFFFFFF]) for h, r in zip(hdr, rec)]
    h, top = sim.roll_now(_ffi.ROLL_TOP_MAX, _ffi.ROLL_BY_ACCUSED)
    out["worst_accusers_at_end"] = nodes(top[:int(h["listed"]) & 0xFFFFFFFF])
    return out


class LedgerRun:
    """--ledger: one ledger per burst of user events until LEDGER_MAX rumours have been followed."""

    def __init__(self, args, sim):
        from serf_amd import _ffi
        self.ffi, self.args, self.sim = _ffi, args, sim
        self.followed, self.open_at, self.done, self.dropped = 0, None, [], 0

    def close(self):
        if self.open_at is None:
            return
        self.dropped += self.sim.ledger_count()[1]
        hdr, rec = self.sim.ledger_read()
        for s in self.ffi.ledger_summary(hdr, rec):
            self.done.append({"injected_at": self.open_at, "samples": len(hdr), **s})
        self.sim.ledger_stop()
        self.open_at = None

    def burst(self, t, rumours):
        """rumours: (kind, key, ltime) of the events about to be injected at tick t."""
        if self.followed >= self.ffi.LEDGER_MAX:
            return
        self.close()
        take = rumours[:self.ffi.LEDGER_MAX - self.followed]
        self.sim.ledger_start(take, 0, self.args.ledger, 1 << 12)
        self.open_at, self.followed = int(t), self.followed + len(take)

    def json(self):
        self.close()
        return {"period": self.args.ledger, "rumours": self.done, "dropped": self.dropped,
                "what": "include/serf_sim_ledger.h: per followed user event (the first 64, a ledger per burst, ended by the next burst): "
                        "first_tick = sim_tick of the first sample with any reach or carriage; reach / running = at the ledger's last "
                        "sample; copies = the sum of the in-flight column (period 1: the copies the cluster sent); died_at = sim_tick "
                        "of the last sample with a copy queued or in flight when a later sample exists; copies_per_node = copies / reach"}


class SpreadRun:
    """--spread: one spread map per burst of user events until SPREAD_MAX rumours have been followed."""

    def __init__(self, args, sim):
        from serf_amd import _ffi
        self.ffi, self.args, self.sim = _ffi, args, sim
        self.followed, self.open_at, self.done, self.dropped = 0, None, [], 0

    def close(self):
        if self.open_at is None:
            return
        taken, dropped = self.sim.spread_count()
        self.dropped += dropped
        for i, s in enumerate(self.sim.spread_summary(1)):
            bins = [int(x) for x in s["bins"]]
            while bins and not bins[-1]:
                bins.pop()
            pct = self.ffi.spread_percentiles(self.sim.spread_map(i), (50, 90, 99, 100))
            self.done.append({"injected_at": self.open_at, "samples": int(taken), "key": int(s["id"] & 0xFFFFFFFF), "ltime": int(s["val"]),
                              "first": int(s["first"]), "last": int(s["last"]), "reached": int(s["reached"]), "reached_up": int(s["reached_up"]),
                              "unreached_up": int(s["unreached_up"]), "mean_delay": float(s["late_sum"]) / int(s["reached"]) if s["reached"] else None,
                              "arrival_percentiles": dict(zip(("50", "90", "99", "100"), pct)), "histogram": bins})
        self.sim.spread_stop()
        self.open_at = None

    def burst(self, t, rumours):
        """rumours: (kind, key, ltime) of the events about to be injected at tick t."""
        if self.followed >= self.ffi.SPREAD_MAX:
            return
        self.close()
        take = rumours[:self.ffi.SPREAD_MAX - self.followed]
        self.sim.spread_start(take, 0, self.args.spread, 1 << 12)
        self.open_at, self.followed = int(t), self.followed + len(take)

    def json(self):
        self.close()
        return {"period": self.args.spread, "rumours": self.done, "dropped": self.dropped,
                "what": "include/serf_sim_spread.h: per followed user event (the first 64, a map per burst, ended by the next burst): first / "
                        "last = the smallest / largest arrival (sim_tick); reached = nodes with an arrival; unreached_up = running nodes "
                        "without one when the map ended; histogram = reached nodes by arrival - first, a tick a bin, the 32nd taking "
                        "everything beyond; arrival_percentiles = the tick by which that share of the reached nodes had it"}


class TreeRun:
    """--tree: one rumour tree per burst of user events until TREE_MAX rumours have been followed."""

    def __init__(self, args, sim):
        from serf_amd import _ffi
        self.ffi, self.args, self.sim = _ffi, args, sim
        self.followed, self.open_at, self.done, self.dropped = 0, None, [], 0

    def close(self):
        if self.open_at is None:
            return
        taken, dropped = self.sim.tree_count()
        self.dropped += dropped
        for i, s in enumerate(self.sim.tree_summary()):
            bins = [int(x) for x in s["hop_bins"]]
            while bins and not bins[-1]:
                bins.pop()
            hops = self.ffi.tree_hops(self.sim.tree_links(i))
            self.done.append({"injected_at": self.open_at, "samples": int(taken), "key": int(s["id"] & 0xFFFFFFFF), "ltime": int(s["val"]),
                              "reached": int(s["reached"]), "orphans": int(s["orphans"]), "orphan_share": hops["orphan_share"],
                              "depth": int(s["depth"]), "mean_hop": hops["mean_hop"],
                              "hop_percentiles": {str(q): v for q, v in hops["percentiles"].items()}, "hop_histogram": bins,
                              "most_children": [{"node": int(r["id"]), "running": int(r["running"]), "children": int(r["link"]["children"]),
                                                 "hop": int(r["link"]["hop"]), "arrival": int(r["link"]["arrival"])}
                                                for r in self.sim.tree_top(i, 10)]})
        self.sim.tree_stop()
        self.open_at = None

    def burst(self, t, rumours):
        """rumours: (kind, key, ltime) of the events about to be injected at tick t."""
        if self.followed >= self.ffi.TREE_MAX:
            return
        self.close()
        take = rumours[:self.ffi.TREE_MAX - self.followed]
        self.sim.tree_start(take, 0, 1 << 12)
        self.open_at, self.followed = int(t), self.followed + len(take)

    def json(self):
        self.close()
        return {"rumours": self.done, "dropped": self.dropped,
                "what": "include/serf_sim_tree.h: per followed user event (the first 64, a tree per burst, ended by the next burst): reached = "
                        "nodes with an arrival; orphans = of them without a parent (the origin, push-pull deliveries); depth = the largest hop "
                        "count; hop_histogram = reached nodes by hop count, the 32nd bin taking everything beyond; hop_percentiles = the hop "
                        "count within which that share of the reached nodes lies; most_children = the ten nodes that were the first to tell "
                        "the most others"}


def census_json(args, sim):
    """The headers of the run's census, one list per field of _ffi.CENSUS_HEADER_DTYPE, and the records of the state at the end."""
    taken, dropped = sim.census_count()
    hdr, _ = sim.census_read()
    out = {"period": args.census, "samples": int(taken), "dropped": int(dropped),
           "what": "include/serf_sim_census.h: state after the tick `tick` - 1; subjects = nodes that own a view slot, observers = running "
                   "nodes; settled = subjects every observer holds the same entry of; false_failed / suspected_running = RUNNING subjects "
                   "somebody holds Failed / Suspect or Dead (*_pairs: how many observers do); stopped_alive = STOPPED subjects somebody "
                   "still holds Alive; detected = stopped subjects every observer holds Failed or Left"}
    for name in hdr.dtype.names:
        if name not in ("reserved", "stored"):
            out[name] = hdr[name].tolist()
    sub = [int(x) for x in hdr["subjects"]]
    out["settled_share"] = [round(int(s) / n, 4) if n else None for s, n in zip(hdr["settled"], sub)]
    _, rec = sim.census_now(64)
    out["at_end"] = [{"subject": int(r["id"]) & 0xFFFFFFFF, "slot": int(r["id"]) >> 32, "running": int(r["running"]),
                      "status": r["status"].tolist(), "swim": r["swim"].tolist(), "intents": int(r["intents"]),
                      "ltime": [int(r["ltime_min"]), int(r["ltime_max"])], "inc": [int(r["inc_min"]), int(r["inc_max"])]} for r in rec]
    return out


def detect_json(args, sim):
    """The run's detection log: _ffi.detect_summary over every episode (closed and still open), the last header, the counts."""
    from serf_amd import _ffi
    import numpy as np
    taken, dropped = sim.detect_count()
    written, lost = sim.detect_log_count()
    log, still = sim.detect_log(), sim.detect_open()
    hdr = sim.detect_read(taken - 1, 1)[0] if taken else None
    return {"period": args.detect, "samples": int(taken), "dropped": int(dropped), "log_written": int(written), "log_lost": int(lost),
            "open_at_end": int(len(still)),
            "what": "include/serf_sim_detect.h: every subject with a view slot, nobody named in advance; a DOWN episode runs from the first "
                    "sample that sees the subject stopped until every running node holds it Failed or Left (detected), it runs again "
                    "(returned) or its slot goes to somebody else (abandoned); an ACCUSED episode from the first sample at which a running "
                    "subject is held Suspect, Dead or Failed by anybody until nobody does (cleared) or it stops; latencies in ticks from "
                    "`opened`, censored episodes (open at the log's first sample) apart; histogram bin of x: 0 for 0, else min(15, 1 + "
                    "floor(log2 x))",
            "summary": _ffi.detect_summary(np.concatenate([log, still])),
            "last_header": None if hdr is None else {name: (hdr[name].tolist() if hdr[name].ndim else int(hdr[name])) for name in hdr.dtype.names}}


def gazette_json(args, sim):
    """The run's member gazette: the per-tick event rates and the flap count (_ffi.gazette_rates), the ten nodes that saw the most
    `failed` events and the ten subjects most often announced failed."""
    import numpy as np
    from serf_amd import _ffi
    taken, dropped = sim.gazette_count()
    s, nodes = sim.gazette_read(), sim.gazette_nodes()
    rates = _ffi.gazette_rates(s, nodes)
    top = lambda which: [{"id": int(r["id"]), **{name: int(r["row"][k]) for k, name in enumerate(_ffi.GAZETTE_COLUMNS)}}
                         for r in sim.gazette_top(which, _ffi.GAZETTE_FAILED, 10)]
    out = {"period": args.gazette, "samples": taken, "dropped": dropped,
           "what": "include/serf_sim_gazette.h: the member events every running node's application was handed, by view diffs behind "
                   "the sampled ticks; per_tick: events per tick over the sampled span; per_node: events of columns 0-3 a node saw",
           "totals": rates["totals"], "per_tick": rates["per_tick"], "flaps": rates["totals"]["flap"], "per_node": rates["per_node"],
           "dead_time_bins": s["dead_time"].astype(np.int64).sum(axis=0).tolist() if len(s) else [],
           "nodes_most_failed": top(_ffi.GAZETTE_MAP_NODES), "subjects_most_failed": top(_ffi.GAZETTE_MAP_SUBJECTS)}
    sim.gazette_stop()
    return out


def catalog_json(args, sim):
    """The run's rumour catalogue: what the registry holds by kind (_ffi.catalog_summary), the identities nobody named — every
    record that is not one of the tool's own user events — and the live curve."""
    from serf_amd import _ffi
    taken, dropped = sim.catalog_count()
    s, reg = sim.catalog_read(), sim.catalog_list()
    summ = _ffi.catalog_summary(reg)
    unnamed = [d for d in summ["identities"] if not (d["kind"] == _ffi.K_EVENT and d["key"] >> 24 == 0x40)]
    by_kind = {}
    for d in unnamed:
        by_kind[d["kind"]] = by_kind.get(d["kind"], 0) + 1
    sim.catalog_stop()
    return {"period": args.catalog, "samples": taken, "dropped": dropped,
            "what": "include/serf_sim_catalog.h: the record identities found live behind the sampled ticks; by_kind: kind -> identities "
                    "in the registry, copies sent for them (period 1), longest life in ticks; unnamed_by_kind: those that are not the "
                    "tool's own user events",
            "registry": len(reg), "ids_lost": int(s["ids_lost"][-1]) if len(s) else 0, "overflowed_samples": int(s["overflowed"][-1]) if len(s) else 0,
            "by_kind": {str(k): v for k, v in summ["by_kind"].items()}, "unnamed_by_kind": {str(k): v for k, v in sorted(by_kind.items())},
            "live_max": int(s["live"].max()) if len(s) else 0, "live_by_kind_max": s["live_by_kind"].max(axis=0).tolist() if len(s) else [],
            "tick": s["tick"].tolist(), "live": s["live"].tolist(), "new": s["new"].tolist(), "died": s["died"].tolist()}


def traffic_json(args, sim):
    """The run's traffic meter: per-node byte rates, the hottest receivers, what went to stopped processes, the in-degree histogram."""
    from serf_amd import _ffi
    taken, dropped = sim.traffic_count()
    s = sim.traffic_read()
    nodes = sim.traffic_nodes()
    rates = _ffi.traffic_rates(nodes, int(taken))
    for side in ("tx_stats", "rx_stats"):
        st = rates[side]
        st["p99_over_median"] = st["p99"] / st["median"] if st["median"] else None
    packets, to_down = int(s["packets"].sum()), int(s["to_down"].sum())
    summ = sim.traffic_summary(5, 64)
    return {"period": args.traffic, "samples": int(taken), "dropped": int(dropped),
            "what": "include/serf_sim_traffic.h: a packet = one (sender, fan-out slot) in flight behind a sampled tick with at least one record; "
                    "bytes = 16-byte units of its records; addressed = to the slot's target, running or not; rates: a sample stands for one "
                    "gossip interval of 200 ms; to_stopped = packets whose target does not run when the sample is taken; degree_bins[b] = "
                    "(node, sample) pairs with min(packets addressed, 31) == b",
            "packets": packets, "records": int(s["records"].sum()), "bytes": 16 * int(s["units"].sum()),
            "to_stopped": to_down, "to_stopped_share": to_down / packets if packets else None,
            "bytes_per_s_sent": rates["tx_stats"], "bytes_per_s_addressed": rates["rx_stats"],
            "most_addressed_in_one_sample": int(s["max_packets"].max()) if len(s) else 0,
            "degree_bins": s["degree_bins"].sum(axis=0).tolist() if len(s) else [],
            "hottest_receivers": [{"node": int(r["id"]), "running": int(r["running"]), **{k: int(r["node"][k]) for k in _ffi.TRAFFIC_COLUMN_NAMES}}
                                  for r in sim.traffic_top(10, 5)],
            "rx_units_summary": {k: (summ[k].tolist() if summ[k].ndim else int(summ[k])) for k in summ.dtype.names}}


def run_tracker(args, sim, lib):
    """The --tracker run: everything the host does happens between two long sim_step calls."""
    import math

    import numpy as np
    from serf_amd import _ffi
    n, total = args.nodes, args.ticks
    NEVER = _ffi.TRACK_NEVER
    FAILED, SUSPECT_OR_DEAD = 1 << _ffi.STATUS_FAILED, 1 << _ffi.SWIM_SUSPECT | 1 << _ffi.SWIM_DEAD
    rng = np.random.default_rng(5)
    # a crashed node is a running suspicion at every node for about the minimum suspicion timeout (memberlist: suspicion_mult x
    # log10 n x probe interval; make_config's suspicion_mult is 4) and some ticks until the first probe finds it
    window = int(4 * max(1.0, math.log10(n)) * args.probe_interval) + 4 * args.probe_interval
    crashes, recent, gone = [], [], set()   # (tick, node)
    for t in range(20, total - args.down - 50):
        recent = [x for x in recent if x + window > t]
        if rng.random() < args.crash_prob and len(recent) < args.crash_cap:
            node = int(rng.integers(0, n))
            while node in gone:
                node = int(rng.integers(0, n))
            gone.add(node)
            crashes.append((t, node))
            recent.append(t)
    for t, node in crashes:
        sim.inject(t, _ffi.OP_CRASH, node)
        sim.inject(t + args.down, _ffi.OP_JOIN, node)
    sample = []
    while len(sample) < args.fp_sample:
        x = int(rng.integers(0, n))
        if x not in gone and x not in sample:
            sample.append(x)
    fp_ids = sim.track_add([_ffi.member_tracker(x, FAILED, SUSPECT_OR_DEAD) for x in sample]) if sample else []
    crash_ids = {}   # node -> (tick, suspect+ id, failed id); registered up front in batches that fit beside the events'
    bursts = max(1, args.rumors // args.burst)
    every = max(1, (total - 100) // bursts)
    live_ev, done_ev, done_cr = [], [], []   # (id, inject tick) / (inject tick, result) / (crash tick, suspect+, failed)
    ci = 0
    ledger = LedgerRun(args, sim) if args.ledger else None
    spread = SpreadRun(args, sim) if args.spread else None
    tree = TreeRun(args, sim) if args.tree else None
    t0 = time.perf_counter()
    stretches = 0

    def harvest(now):
        nonlocal live_ev
        over = [(i, t) for i, t in live_ev if t + args.max_rounds <= now]
        if over:
            for (i, t), r in zip(over, sim.track_read([i for i, _ in over])):
                done_ev.append((t, r.as_dict()))
            sim.track_remove([i for i, _ in over])
            live_ev = [(i, t) for i, t in live_ev if t + args.max_rounds > now]
        ended = [node for node, (t, a, b) in crash_ids.items() if t + args.down <= now]
        if ended:
            ids = [x for node in ended for x in crash_ids[node][1:]]
            rs = sim.track_read(ids)
            for k, node in enumerate(ended):
                done_cr.append((crash_ids[node][0], rs[2 * k].as_dict(), rs[2 * k + 1].as_dict()))
                del crash_ids[node]
            sim.track_remove(ids)

    while sim.tick < total:
        t = sim.tick
        harvest(t)
        # the crashes of the coming stretch get their two trackers now (their windows open at the crash)
        batch = []
        while ci < len(crashes) and crashes[ci][0] < t + every:
            batch.append(crashes[ci])
            ci += 1
        if batch:
            ids = sim.track_add([tr for ct, node in batch for tr in (_ffi.member_tracker(node, FAILED, SUSPECT_OR_DEAD, start=ct, max_age=args.down),
                                                                     _ffi.member_tracker(node, FAILED, start=ct, max_age=args.down))])
            for k, (ct, node) in enumerate(batch):
                crash_ids[node] = (ct, ids[2 * k], ids[2 * k + 1])
        if 50 <= t < total - args.max_rounds:
            specs, keys = [], []
            for _ in range(args.burst):
                node = int(rng.integers(0, n))
                while node in gone:
                    node = int(rng.integers(0, n))
                key = 0x40000000 + len(done_ev) + len(live_ev) + len(keys)
                specs.append(_ffi.rumour_tracker(_ffi.K_EVENT, key, sim.stats(node).event_time, max_age=args.max_rounds))
                keys.append((node, key))
            live_ev += [(i, t) for i in sim.track_add(specs)]
            if ledger:
                ledger.burst(t, [(sp.a, sp.b, sp.ltime) for sp in specs])
            if spread:
                spread.burst(t, [(sp.a, sp.b, sp.ltime) for sp in specs])
            if tree:
                tree.burst(t, [(sp.a, sp.b, sp.ltime) for sp in specs])
            for node, key in keys:
                sim.user_event(node, key, 64)
        sim.step(min(every, total - t))     # ONE call per stretch; nothing is read back inside it
        stretches += 1
    sim.sync()
    dt = time.perf_counter() - t0
    harvest(sim.tick + args.max_rounds + args.down)
    fp = [r.as_dict() for r in sim.track_read(fp_ids)] if fp_ids else []
    cs = sim.cluster_stats()
    series = series_json(args, sim) if args.series else None
    census = census_json(args, sim) if args.census else None
    roll = roll_json(args, sim) if args.roll else None
    ledger = ledger.json() if ledger else None
    spread = spread.json() if spread else None
    tree = tree.json() if tree else None
    detect = detect_json(args, sim) if args.detect else None
    traffic = traffic_json(args, sim) if args.traffic else None
    catalog = catalog_json(args, sim) if args.catalog else None
    gazette = gazette_json(args, sim) if args.gazette else None

    def rounds(name):
        return [r[name] - t for t, r in done_ev if r[name] != NEVER]
    out = {
        "what": "BASELINE configs[4] on one GPU followed by device-resident trackers: crashes with a per-tick probability, user events in bursts "
                "while the churn runs, one sim_step per stretch; latencies in ticks",
        "config": {k: v for k, v in vars(args).items() if k not in ("out", "lib")}, "backend": lib.backend_name(),
        "ticks": int(sim.tick), "sim_step_calls": stretches, "crashes": len(crashes), "suspicion_window_assumed": window,
        "events": len(done_ev),
        "rounds_to": {k: {"histogram": hist(rounds(f)), "not_reached": sum(r[f] == NEVER for _, r in done_ev)}
                      for k, f in (("50", "half"), ("90", "p90"), ("99", "p99"), ("100", "all"))},
        "detection": {
            "crashes_followed": len(done_cr),
            "first_suspicion_after_crash": {"histogram": hist([a["first"] - t for t, a, b in done_cr if a["first"] != NEVER]),
                                            "never": sum(a["first"] == NEVER for t, a, b in done_cr)},
            "declared_failed_by_99pct_after_crash": {"histogram": hist([b["p99"] - t for t, a, b in done_cr if b["p99"] != NEVER]),
                                                     "never": sum(b["p99"] == NEVER for t, a, b in done_cr)}},
        "false_positives": {"sampled_never_crashed_nodes": len(fp), "ever_suspected_or_worse_by_anybody": sum(r["peak"] > 0 for r in fp),
                            "largest_number_of_accusers": max([r["peak"] for r in fp], default=0)},
        "model_bound_drops": int(cs["overflow"]), "ops_dropped_no_slot": int(cs["ops_dropped"]),
        "view_slots_recycled": int(cs["slots_recycled"]), "nodes_up_at_end": int(cs["up"]),
        "wall_s": dt, "member_ticks_per_s_incl_tracking": n * int(sim.tick) / dt,
    }
    if series:
        out["series"] = series
    if census:
        out["census"] = census
    if roll:
        out["roll"] = roll
    if ledger:
        out["ledger"] = ledger
    if spread:
        out["spread"] = spread
    if tree:
        out["tree"] = tree
    if detect:
        out["detect"] = detect
    if traffic:
        out["traffic"] = traffic
    if catalog:
        out["catalog"] = catalog
    if gazette:
        out["gazette"] = gazette
    json.dump(out, open(args.out, "w"), indent=None if series or census or roll else 1)
    print(json.dumps({k: out[k] for k in ("ticks", "sim_step_calls", "crashes", "events", "false_positives", "model_bound_drops", "ops_dropped_no_slot", "wall_s")}), "->", args.out)
    print(json.dumps({"rounds_to_99": out["rounds_to"]["99"], "detection": out["detection"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1 << 20)
    ap.add_argument("--fanout", type=int, default=4)
    ap.add_argument("--loss", type=float, default=0.01)
    ap.add_argument("--churn-frac", type=float, default=0.05)
    ap.add_argument("--churn-every", type=int, default=24, help="ticks between two crashes")
    ap.add_argument("--down", type=int, default=160, help="ticks a crashed node stays down before it re-joins")
    ap.add_argument("--rumors", type=int, default=1000)
    ap.add_argument("--view-slots", type=int, default=1024)
    ap.add_argument("--ring", type=int, default=512)
    ap.add_argument("--probe-interval", type=int, default=5)
    ap.add_argument("--push-pull-interval", type=int, default=150)
    ap.add_argument("--recycle-interval", type=int, default=75)
    ap.add_argument("--pkt-records", type=int, default=4)
    ap.add_argument("--max-rounds", type=int, default=60)
    ap.add_argument("--random-fanout", action="store_true", help="gossip targets by memberlist's literal kRandomNodes (explicit per-tick CSR) instead of the bijection")
    ap.add_argument("--tcp-fallback", action="store_true", help="memberlist's stream-transport fallback ping (its default): packet loss alone never fails a probe")
    ap.add_argument("--nacks", action="store_true", help="memberlist's nack accounting for the health score")
    ap.add_argument("--reconnect-interval", type=int, default=0, help="Reconnector period in ticks (reference: 30 s = 150; 0 = off)")
    ap.add_argument("--gossip-to-the-dead", type=int, default=0, help="memberlist gossip_to_the_dead_time in ticks (lan: 30 s = 150; 0 = off)")
    ap.add_argument("--ring-overflow", type=int, default=8, help="overflow rows per de-dup ring and node (sim_config.ring_overflow)")
    ap.add_argument("--vshards", type=int, default=1, help="virtual shards of the fan-out map (the shape of one rank's share of a V-way sharded cluster)")
    ap.add_argument("--chunks", type=int, default=0, help="sender chunks per shard (the chunk-wise exchange's layout)")
    ap.add_argument("--lib", default=None, help="oracle: run the CPU oracle instead (small sizes; for checking the tool)")
    ap.add_argument("--tracker", action="store_true", help="follow the run with device-resident trackers (see above) instead of polling every tick")
    ap.add_argument("--ticks", type=int, default=4000, help="--tracker: length of the run")
    ap.add_argument("--crash-prob", type=float, default=1 / 24, help="--tracker: probability per tick that one running node crashes")
    ap.add_argument("--crash-cap", type=int, default=10, help="--tracker: crashes inside one suspicion window (SIM_S = 16 timers per node, some are false suspicions)")
    ap.add_argument("--burst", type=int, default=4, help="--tracker: user events injected at once (they share a Lamport time, hence a ring bucket of SIM_C = 6 keys: more than 6 use up the overflow rows)")
    ap.add_argument("--fp-sample", type=int, default=64, help="--tracker: never-crashed nodes watched for false suspicions")
    ap.add_argument("--series", type=int, default=0, metavar="PERIOD", help="sample the cluster gauges on the device behind every PERIOD-th tick (include/serf_sim_series.h) and put the series into the JSON")
    ap.add_argument("--census", type=int, default=0, metavar="PERIOD", help="count the views of every subject with a view slot on the device behind every PERIOD-th tick (include/serf_sim_census.h) and put the agreement curves into the JSON")
    ap.add_argument("--roll", type=int, default=0, metavar="PERIOD", help="measure every running node's view against the per-subject references on the device behind every PERIOD-th tick (include/serf_sim_roll.h) and put the curves and the worst observers into the JSON")
    ap.add_argument("--ledger", type=int, default=0, metavar="PERIOD", help="--tracker: follow the first 64 user events with rumour ledgers, sampled behind every PERIOD-th tick (include/serf_sim_ledger.h), and put their summaries into the JSON")
    ap.add_argument("--spread", type=int, default=0, metavar="PERIOD", help="--tracker: follow the first 64 user events with spread maps, latched behind every PERIOD-th tick (include/serf_sim_spread.h), and put their arrival histograms and unreached counts into the JSON")
    ap.add_argument("--detect", type=int, default=0, metavar="PERIOD", help="judge every subject with a view slot on the device behind every PERIOD-th tick (include/serf_sim_detect.h): the episodes of every crash and every accusation of the run, their summary into the JSON")
    ap.add_argument("--tree", action="store_true", help="--tracker: follow the first 64 user events with rumour trees, latched behind every tick (include/serf_sim_tree.h), and put their hop histograms, depths, orphans and the ten nodes with the most children into the JSON")
    ap.add_argument("--traffic", type=int, default=0, metavar="PERIOD", help="meter the gossip packets per sender and per target on the device behind every PERIOD-th tick (include/serf_sim_traffic.h): per-node byte percentiles and the ten hottest receivers into the JSON")
    ap.add_argument("--gazette", type=int, default=0, metavar="PERIOD", help="count every node's member events on the device behind every PERIOD-th tick (include/serf_sim_gazette.h): the per-tick rates, the flaps, the ten nodes that saw the most failed events and the ten subjects most often announced failed into the JSON")
    ap.add_argument("--catalog", type=int, default=0, metavar="PERIOD", help="find the live record identities on the device behind every PERIOD-th tick (include/serf_sim_catalog.h): the registry by kind, the identities nobody named and the live curve into the JSON")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.ledger and not args.tracker:
        ap.error("--ledger follows the rumours of a --tracker run")
    if args.spread and not args.tracker:
        ap.error("--spread follows the rumours of a --tracker run")
    if args.tree and not args.tracker:
        ap.error("--tree follows the rumours of a --tracker run")
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r17_config4_catalog.json" if args.catalog else "r15_config4_tree.json" if args.tree else "r14_config4_traffic.json" if args.traffic else "r12_config4_detect.json" if args.detect else "r13_config4_spread.json" if args.spread else "r11_config4_ledger.json" if args.ledger else "r10_config4_roll.json" if args.roll else "r09_config4_census.json" if args.census else "r08_config4_series.json" if args.series else "r07_config4_tracker.json" if args.tracker else "r03_config4_churn5_loss1_swim.json")

    import numpy as np
    from serf_amd import _ffi

    if args.lib == "oracle":
        from tests._oracle import load_oracle
        lib = load_oracle()
    else:
        import serf_amd
        lib = serf_amd.load()
    n = args.nodes
    kw = dict(fanout=args.fanout, view_slots=args.view_slots, event_ring=args.ring, query_ring=args.ring,
              probe_interval=args.probe_interval, push_pull_interval=args.push_pull_interval, loss=args.loss,
              reap_interval=75, queue_check_interval=150, recycle_interval=args.recycle_interval, pkt_records=args.pkt_records,
              reconnect_interval=args.reconnect_interval, gossip_to_the_dead=args.gossip_to_the_dead,
              tcp_fallback=args.tcp_fallback, nacks=args.nacks, vshards=args.vshards, chunks=args.chunks, ring_overflow=args.ring_overflow,
              **({"flags": _ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT} if args.random_fanout else {}),
              join_sync=True)   # Serf::join = memberlist.join: the re-joining node syncs with a peer (SIM_CF_JOIN_SYNC)
    sim = _ffi.Sim(lib, _ffi.make_config(n, **kw))
    if args.series:
        sim.series_start(0, args.series, min(_ffi.SERIES_MAX_SAMPLES, 1 << 16))
    if args.census:
        sim.census_start(0, args.census, min(_ffi.CENSUS_MAX_SAMPLES, 1 << 16), 1)   # (the headers' curves: one record a sample is the least)
    if args.roll:
        sim.roll_start(0, args.roll, min(_ffi.ROLL_MAX_SAMPLES, 1 << 16), ROLL_TOP, _ffi.ROLL_BY_STALE)
    if args.detect:
        sim.detect_start(0, args.detect, min(_ffi.DETECT_MAX_SAMPLES, 1 << 16), 1 << 20)
    if args.traffic:
        sim.traffic_start(0, args.traffic, min(_ffi.TRAFFIC_MAX_SAMPLES, 1 << 16))
    if args.catalog:
        sim.catalog_start(_ffi.CATALOG_KINDS, _ffi.CATALOG_MAX, 0, args.catalog, min(_ffi.CATALOG_MAX_SAMPLES, 1 << 16))
    if args.gazette:
        sim.gazette_start(0, args.gazette, min(_ffi.GAZETTE_MAX_SAMPLES, 1 << 16), 60)
    if args.tracker:
        return run_tracker(args, sim, lib)
    rng = np.random.default_rng(5)
    n_churn = int(n * args.churn_frac)
    total = 20 + n_churn * args.churn_every + args.down + 400
    churned = rng.choice(n, n_churn, replace=False)
    crash_at = 20 + np.arange(n_churn) * args.churn_every
    for t, node in zip(crash_at.tolist(), churned.tolist()):
        sim.inject(t, _ffi.OP_CRASH, node)
        sim.inject(t + args.down, _ffi.OP_JOIN, node)
    down = {int(node): (int(t), int(t) + args.down) for t, node in zip(crash_at.tolist(), churned.tolist())}
    every = max(1, (total - 100) // args.rumors)
    rumor_ticks = [50 + i * every for i in range(args.rumors)]
    rounds, outstanding = [], {}
    stats = {"max_failed_entries": 0, "max_slots_in_use": 0, "max_queue": 0}
    t0 = time.perf_counter()
    ri = 0
    while sim.tick < total:
        t = sim.tick
        nxt = rumor_ticks[ri] if ri < len(rumor_ticks) else total
        if not outstanding and t < nxt:     # nothing to watch: run ahead to the next rumour
            sim.step(min(nxt, total) - t)
            cs = sim.cluster_stats()
            stats["max_failed_entries"] = max(stats["max_failed_entries"], int(cs["failed"]))
            stats["max_slots_in_use"] = max(stats["max_slots_in_use"], int(cs["slots_in_use"]))
            stats["max_queue"] = max(stats["max_queue"], int(cs["max_queue"]))
            continue
        if ri < len(rumor_ticks) and t == rumor_ticks[ri]:
            node = int(rng.integers(0, n))
            while node in down and down[node][0] - 2 <= t <= down[node][1] + 2:
                node = int(rng.integers(0, n))
            key = 0x40000000 + ri
            outstanding[key] = (sim.stats(node).event_time, t)
            sim.user_event(node, key, 64)
            ri += 1
        sim.step(1)
        keys = list(outstanding)
        seen, up = sim.convergence_many([(_ffi.K_EVENT, k, outstanding[k][0]) for k in keys])
        for k, s in zip(keys, seen):
            r = sim.tick - outstanding[k][1]
            if s * 100 >= up * 99:
                rounds.append(r)
                del outstanding[k]
            elif r > args.max_rounds:
                rounds.append(args.max_rounds + 1)
                del outstanding[k]
    sim.sync()
    dt = time.perf_counter() - t0
    r = np.array(rounds)
    rows = sim.dump(_ffi.ARR_ROWS)
    cs = sim.cluster_stats()
    ev_failed = int((rows["n_failed"] > 0).sum())
    out = {
        "what": "BASELINE configs[4] on one GPU: churn + packet loss with the SWIM layer on; rounds until >= 99 % of the running nodes have "
                "applied a user event",
        "config": {k: v for k, v in vars(args).items() if k not in ("out", "lib", "tracker", "ticks", "crash_prob", "crash_cap", "burst", "fp_sample", "series", "census", "roll", "ledger", "detect", "spread", "traffic", "tree", "catalog", "gazette")},
        "backend": lib.backend_name(),
        "ticks": int(sim.tick), "churn_events": int(n_churn), "churn_frac_of_nodes": n_churn / n, "rumors": int(len(r)),
        "rounds_to_99": {"median": float(np.median(r)), "p90": float(np.percentile(r, 90)), "p99": float(np.percentile(r, 99)),
                         "max": int(r.max()), "min": int(r.min()), "not_converged": int((r > args.max_rounds).sum())},
        "histogram": {int(k): int(v) for k, v in zip(*np.unique(r, return_counts=True))},
        "failure_detector": {"max_failed_entries_seen_cluster_wide": stats["max_failed_entries"],
                             "nodes_still_holding_a_failed_entry_at_end": ev_failed,
                             "refutations_incarnation_sum": int(rows["inc"].sum()),
                             "nodes_that_refuted": int((rows["inc"] > 0).sum()),
                             "awareness_nonzero_at_end": int((rows["awareness"] > 0).sum())},
        "model_bound_drops": int(cs["overflow"]), "ops_dropped_no_slot": int(cs["ops_dropped"]),
        "view_slots_recycled": int(cs["slots_recycled"]), "view_slots_in_use_at_end": int(cs["slots_in_use"]),
        "max_view_slots_in_use_seen": stats["max_slots_in_use"], "deepest_queue_seen": stats["max_queue"],
        "nodes_up_at_end": int(cs["up"]), "wall_s": dt, "member_ticks_per_s_incl_host_polling": n * int(sim.tick) / dt,
    }
    try:
        import torch
        free, tot = torch.cuda.mem_get_info()
        out["device_memory"] = {"in_use_bytes_at_end": int(tot - free), "total_bytes": int(tot),
                                "what": "hipMemGetInfo at the end of the run: this handle's arrays (views, rings, packets, rows) and the runtime's own"}
    except Exception:
        pass
    if args.series:
        out["series"] = series_json(args, sim)
    if args.census:
        out["census"] = census_json(args, sim)
    if args.roll:
        out["roll"] = roll_json(args, sim)
    if args.detect:
        out["detect"] = detect_json(args, sim)
    if args.traffic:
        out["traffic"] = traffic_json(args, sim)
    if args.catalog:
        out["catalog"] = catalog_json(args, sim)
    if args.gazette:
        out["gazette"] = gazette_json(args, sim)
    json.dump(out, open(args.out, "w"), indent=None if args.series or args.census or args.roll else 1)
    print(json.dumps({k: out[k] for k in ("ticks", "churn_events", "rounds_to_99", "model_bound_drops", "ops_dropped_no_slot", "failure_detector", "wall_s")}), "->", args.out)


if __name__ == "__main__":
    main()
