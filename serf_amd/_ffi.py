"""ctypes binding of the C ABI declared in include/serf_sim.h.

The binding is generic over (shared-library path, symbol prefix): the product library
``serf_amd/csrc/libserf_sim.so`` exports ``sim_*``; a test may bind any other implementation of
the same ABI (the CPU oracle exports ``osim_*``) by passing its own path — nothing in this package
knows where such a library lives.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

P, Q, CKEYS, MAX_FANOUT = 4, 64, 6, 4
Q_HOT = 16  # SIM_Q_HOT: the entries the HIP tick kernel keeps in registers
DEFAULT_SEED = 0x5EEDC0DE5E4F0001
STAMP_BITS = 21                             # SIM_STAMP_BITS: a view entry's stamp is the tick modulo 2^21
INTERVAL_LIMIT = 1 << STAMP_BITS            # SIM_INTERVAL_LIMIT: every interval and timeout of the config stays below it
TICK_MAX = (1 << 32) - (1 << 22) - 1        # SIM_TICK_MAX: the last tick a handle executes (a step beyond it: SIM_ERANGE)

OK, EINVAL, ENOMEM, EDEVICE, ENOSLOT, ESTATE, ERANGE, ETOOBIG = 0, -1, -2, -3, -4, -5, -6, -7
_ERR = {EINVAL: "SIM_EINVAL", ENOMEM: "SIM_ENOMEM", EDEVICE: "SIM_EDEVICE", ENOSLOT: "SIM_ENOSLOT",
        ESTATE: "SIM_ESTATE", ERANGE: "SIM_ERANGE", ETOOBIG: "SIM_ETOOBIG"}

# enum sim_member_status (types/member.rs:54-87)
STATUS_NONE, STATUS_ALIVE, STATUS_LEAVING, STATUS_LEFT, STATUS_FAILED = 0, 1, 2, 3, 4
# enum sim_kind
K_JOIN, K_LEAVE, K_EVENT, K_QUERY, K_ALIVE, K_SUSPECT, K_DEAD = 1, 2, 3, 4, 5, 6, 7
# enum sim_event_type (event.rs:263-279, 367-378)
EV_JOIN, EV_LEAVE, EV_FAILED, EV_UPDATE, EV_REAP, EV_USER, EV_QUERY = range(7)
# enum sim_op
OP_USER_EVENT, OP_QUERY, OP_LEAVE, OP_JOIN, OP_FORCE_LEAVE, OP_CRASH, OP_REVIVE, OP_LEAVE_FINISH = 1, 2, 3, 4, 5, 6, 7, 8
OP_SET_TAGS, OP_QUERY_FILTER_ID, OP_QUERY_FILTER_TAGS, OP_DELIVER, OP_SUSPECT, OP_RECONNECT = 9, 10, 11, 12, 13, 14
OP_PRUNE = 17   # internal: the end of handle_prune's wait (CF_PRUNE_DELAY), scheduled by the library from the tick's request list
OP_QRESP, OP_WITNESS = 15, 16   # internal: scheduled by sim_deliver_message (a QueryResponse / a PushPull's clocks), refused by sim_inject
SUSPECT_REQ_MAX, SREQ_HEAD_WORDS = 4096, 8193
QF_IDS, TAG_CLASSES, NO_TAG_FILTER = 12, 32, 0xFFFFFFFF
# enum sim_array
ARR_ROWS, ARR_QUEUE, ARR_INBOX, ARR_VIEW, ARR_ERING, ARR_QRING, ARR_SLOTMAP = range(7)
# enum sim_swim_state (memberlist node state)
SWIM_ALIVE, SWIM_SUSPECT, SWIM_DEAD, SWIM_LEFT = 0, 1, 2, 3
CF_BASELINE_JOINED, CF_RANDOM_FANOUT, CF_AWARENESS_PROBE, CF_JOIN_SYNC, CF_TCP_FALLBACK, CF_NACKS, CF_FORCE_SHARDED, CF_PRUNE_DELAY = 1, 2, 4, 8, 16, 32, 64, 128
XCHG_ALL_TO_ALL, XCHG_ALL_GATHER, XCHG_PACKED = 0, 1, 2   # (ALL_GATHER: retired in ABI 13, never reported)
EXCHANGE_ID_BYTES = 128
F_NO_BROADCAST, F_ACK, F_RESPOND = 1, 2, 4


class SimError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what}: {_ERR.get(code, code)}")
        self.code = code


class Config(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "struct_size", "n_nodes", "vshards", "shard_rank", "shard_count", "fanout", "view_slots",
        "event_ring", "query_ring", "retransmit_mult", "probe_interval", "suspicion_mult",
        "suspicion_max_mult", "indirect_checks", "loss_u32", "intent_timeout", "leave_delay",
        "reap_interval", "reconnect_timeout", "tombstone_timeout", "queue_check_interval", "max_queue_depth",
        "min_queue_depth", "push_pull_interval", "chunks", "recycle_interval", "pkt_records", "flags", "gossip_to_the_dead", "reconnect_interval",
        "ring_overflow", "reserved0")] + [("seed", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("members", C.c_uint32), ("failed", C.c_uint32), ("left", C.c_uint32),
                ("health_score", C.c_uint32), ("member_time", C.c_uint64),
                ("event_time", C.c_uint64), ("query_time", C.c_uint64),
                ("intent_queue", C.c_uint32), ("event_queue", C.c_uint32),
                ("query_queue", C.c_uint32), ("swim_queue", C.c_uint32),
                ("serf_state", C.c_uint32), ("up", C.c_uint32), ("incarnation", C.c_uint32),
                ("queue_overflow", C.c_uint32)]


class ClusterStats(C.Structure):
    _fields_ = [("up", C.c_uint64), ("queued", C.c_uint64 * 4), ("overflow", C.c_uint64),
                ("inbox_records", C.c_uint64), ("failed", C.c_uint64), ("left", C.c_uint64), ("max_queue", C.c_uint64),
                ("ops_dropped", C.c_uint64), ("slots_in_use", C.c_uint64), ("slots_recycled", C.c_uint64),
                ("events_lost", C.c_uint64)]


class RecycleCand(C.Structure):
    _fields_ = [("subject", C.c_uint32), ("slot", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32),
                ("ltime", C.c_uint64), ("inc", C.c_uint32), ("bits", C.c_uint32), ("conf", C.c_uint32 * 4)]


RECYCLE_BATCH = 64


class Event(C.Structure):
    _fields_ = [("tick", C.c_uint32), ("observer", C.c_uint32), ("type", C.c_uint32),
                ("key", C.c_uint32), ("ltime", C.c_uint64)]


ROW_DTYPE = np.dtype([("clock", "<u8"), ("event_clock", "<u8"), ("query_clock", "<u8"),
                      ("event_min", "<u8"), ("query_min", "<u8"), ("flags", "<u4"), ("inc", "<u4"),
                      ("n_known", "<u4"), ("n_failed", "<u4"), ("n_left", "<u4"),
                      ("next_seq", "<u4"), ("overflow", "<u4"), ("susp_next", "<u4"),
                      ("awareness", "<u4"), ("reap_next", "<u4"), ("susp", "<u2", (16,))])
REC_DTYPE = np.dtype([("key", "<u4"), ("meta", "<u4"), ("val", "<u8")])
PACKET_DTYPE = np.dtype([("key", "<u4", (4,)), ("val_lo", "<u4", (4,)), ("hi_meta", "<u4", (4,))])  # 12-byte wire records
VIEW_DTYPE = np.dtype([("ltime", "<u8"), ("inc", "<u4"), ("bits", "<u4"), ("conf", "<u4", (4,))])
BUCKET_DTYPE = np.dtype([("ltime", "<u8"), ("keys", "<u4", (CKEYS,))])
_ARR_DTYPE = {ARR_ROWS: ROW_DTYPE, ARR_QUEUE: REC_DTYPE, ARR_INBOX: PACKET_DTYPE, ARR_VIEW: VIEW_DTYPE,
              ARR_ERING: BUCKET_DTYPE, ARR_QRING: BUCKET_DTYPE, ARR_SLOTMAP: np.dtype("<u4")}

# every symbol include/serf_sim.h declares (without prefix)
ABI_SYMBOLS = ("create", "destroy", "set_stream", "join", "leave", "force_leave", "user_event",
               "query", "inject", "step", "sync", "tick", "members", "stats_get", "watch",
               "drain_events", "state_digest", "dump_state", "convergence", "convergence_many", "exchange_bytes",
               "bind_exchange", "snapshot", "restore", "query_status", "query_responders", "profile", "profile_read", "profile_read_stats", "cluster_stats_get", "resident_planes",
               "bind_exchange2", "bind_exchange3", "exchange_chunks", "exchange_layout", "step_begin", "step_chunk", "step_end",
               "recycle_due", "recycle_scan", "recycle_apply", "pp_due", "pp_plan", "pp_export", "pp_merge",
               "query_filtered", "set_tags", "init_tags", "inject_record", "deliver_message", "user_event_bytes", "peek_packet", "suspect_requests", "suspect_export", "suspect_import",
               "exchange_unique_id", "exchange_init", "exchange_chunk", "exchange_wait", "exchange_library",
               "abi_version", "backend_name")

# include/serf_sim_track.h: device-resident trackers.  An extension with a version of its own, bound only when the loaded
# library exports it (the product does; the CPU oracle, the checker, has none)
TRACK_SYMBOLS = ("track_add", "track_remove", "track_read", "track_active", "track_version")
TRACK_MAX, TRACK_NEVER = 1024, 0xFFFFFFFF
TRK_RUMOUR, TRK_MEMBER = 1, 2


# include/serf_sim_series.h: device-resident time series (cluster gauges sampled behind a tick).  Likewise an extension with a
# version of its own, bound only when the loaded library exports it
SERIES_SYMBOLS = ("series_start", "series_count", "series_read", "series_stop", "series_version")
SERIES_WORDS, SERIES_MAX_SAMPLES = 64, 1 << 20
# one sample as a numpy record: the table of include/serf_sim_series.h, 64 little-endian 64-bit words
SERIES_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("state", "<u8", (4,)), ("queued", "<u8", (4,)),
                         ("depth_bins", "<u8", (8,)), ("max_depth", "<u8"), ("awareness", "<u8", (8,)),
                         ("timers", "<u8"), ("nodes_with_timers", "<u8"), ("n_failed", "<u8"), ("n_left", "<u8"),
                         ("n_known_min", "<u8"), ("n_known_max", "<u8"), ("clock_min", "<u8"), ("clock_max", "<u8"),
                         ("event_clock_min", "<u8"), ("event_clock_max", "<u8"), ("query_clock_min", "<u8"),
                         ("query_clock_max", "<u8"), ("overflow", "<u8"), ("packets", "<u8"), ("records", "<u8", (7,)),
                         ("len64", "<u8"), ("reserved", "<u8", (15,))])
assert SERIES_DTYPE.itemsize == 8 * SERIES_WORDS


# include/serf_sim_census.h: membership census (per subject, how the running nodes' views of it agree).  The third extension:
# a version of its own, bound only when the loaded library exports it
CENSUS_SYMBOLS = ("census_start", "census_count", "census_read", "census_stop", "census_now", "census_version")
CENSUS_WORDS, CENSUS_MAX_SAMPLES = 16, 1 << 20
# a subject's record and a sample's header as numpy records: the tables of include/serf_sim_census.h, 16 little-endian 64-bit
# words each ("id" = subject | slot << 32: subject_of() / slot_of() below take it apart)
CENSUS_SUBJECT_DTYPE = np.dtype([("id", "<u8"), ("running", "<u8"), ("status", "<u8", (5,)), ("swim", "<u8", (4,)),
                                 ("intents", "<u8"), ("ltime_min", "<u8"), ("ltime_max", "<u8"), ("inc_min", "<u8"),
                                 ("inc_max", "<u8")])
CENSUS_HEADER_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("subjects", "<u8"), ("stored", "<u8"), ("settled", "<u8"),
                                ("false_failed", "<u8"), ("false_failed_pairs", "<u8"), ("suspected_running", "<u8"),
                                ("suspected_running_pairs", "<u8"), ("stopped_alive", "<u8"), ("stopped_alive_pairs", "<u8"),
                                ("detected", "<u8"), ("reserved", "<u8", (4,))])
assert CENSUS_SUBJECT_DTYPE.itemsize == CENSUS_HEADER_DTYPE.itemsize == 8 * CENSUS_WORDS


def sample_split(words, hdr_dtype, rec_dtype, per_sample):
    """[samples * (a header + per_sample records)] words -> (headers[samples], records[samples][per_sample])."""
    hw, rw = hdr_dtype.itemsize // 8, rec_dtype.itemsize // 8
    a = np.ascontiguousarray(np.asarray(words, np.uint64)).reshape(-1, hw + per_sample * rw)
    hdr = np.ascontiguousarray(a[:, :hw]).view(hdr_dtype).reshape(-1)
    rec = np.ascontiguousarray(a[:, hw:]).view(rec_dtype).reshape(-1, per_sample)
    return hdr, rec


def census_split(words, max_subjects):
    """[samples * (1 + max_subjects) * 16] words -> (headers[samples], records[samples][max_subjects])."""
    return sample_split(words, CENSUS_HEADER_DTYPE, CENSUS_SUBJECT_DTYPE, max_subjects)


# include/serf_sim_roll.h: observer roll (per running node, how far its view lags and whom it accuses; binned and ranked).  The
# fourth extension: a version of its own, bound only when the loaded library exports it
ROLL_SYMBOLS = ("roll_start", "roll_count", "roll_read", "roll_stop", "roll_now", "roll_version")
ROLL_HEADER_WORDS, ROLL_NODE_WORDS, ROLL_TOP_MAX, ROLL_MAX_SAMPLES = 32, 8, 64, 1 << 20
ROLL_BY_STALE, ROLL_BY_ACCUSED, ROLL_BY_MISSED = 0, 1, 2
# a node's record and a sample's header as numpy records: the tables of include/serf_sim_roll.h ("id" = node | running << 32,
# "listed" = listed | rank_by << 32)
ROLL_NODE_DTYPE = np.dtype([("id", "<u8"), ("stale", "<u8"), ("unknown", "<u8"), ("false_failed", "<u8"), ("suspects", "<u8"),
                            ("stale_alive", "<u8"), ("lag", "<u8"), ("behind", "<u8")])
ROLL_HEADER_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("subjects", "<u8"), ("listed", "<u8"), ("current", "<u8"),
                              ("stale_sum", "<u8"), ("stale_max", "<u8"), ("unknown_sum", "<u8"), ("accusers_failed", "<u8"),
                              ("false_failed_sum", "<u8"), ("accusers_suspect", "<u8"), ("suspects_sum", "<u8"),
                              ("holders_stale_alive", "<u8"), ("stale_alive_sum", "<u8"), ("lag_sum", "<u8"), ("lag_max", "<u8"),
                              ("stale_bins", "<u8", (16,))])
assert ROLL_NODE_DTYPE.itemsize == 8 * ROLL_NODE_WORDS and ROLL_HEADER_DTYPE.itemsize == 8 * ROLL_HEADER_WORDS


def roll_split(words, top_k):
    """[samples * (32 + 8 * top_k)] words -> (headers[samples], records[samples][top_k])."""
    return sample_split(words, ROLL_HEADER_DTYPE, ROLL_NODE_DTYPE, top_k)


# include/serf_sim_ledger.h: rumour ledger (per record identity: reach, queued and in-flight copies behind a tick).  The fifth
# extension: a version of its own, bound only when the loaded library exports it
LEDGER_SYMBOLS = ("ledger_start", "ledger_count", "ledger_read", "ledger_stop", "ledger_now", "ledger_version")
LEDGER_HEADER_WORDS, LEDGER_ENTRY_WORDS, LEDGER_MAX, LEDGER_MAX_SAMPLES = 8, 8, 64, 1 << 20
# a sample's header and one entry's record as numpy records: the tables of include/serf_sim_ledger.h ("id" = key | kind << 32)
LEDGER_HEADER_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("n", "<u8"), ("queued", "<u8"), ("in_flight", "<u8"),
                                ("packets", "<u8"), ("transmits", "<u8"), ("reserved", "<u8")])
LEDGER_ENTRY_DTYPE = np.dtype([("id", "<u8"), ("val", "<u8"), ("reach", "<u8"), ("holders", "<u8"), ("queued", "<u8"),
                               ("transmits", "<u8"), ("in_flight", "<u8"), ("fresh", "<u8")])
assert LEDGER_HEADER_DTYPE.itemsize == 8 * LEDGER_HEADER_WORDS and LEDGER_ENTRY_DTYPE.itemsize == 8 * LEDGER_ENTRY_WORDS


def ledger_split(words, n):
    """[samples * (8 + 8 * n)] words -> (headers[samples], records[samples][n])."""
    return sample_split(words, LEDGER_HEADER_DTYPE, LEDGER_ENTRY_DTYPE, n)


def ledger_summary(headers, records):
    """What a ledger's samples say about each entry, in the entries' order — a list of dicts:
      kind, key, val   the identity
      first_tick       the tick word of the first sample with any reach or carriage (queued + in flight), None when there is none
      reach, running   of the last sample
      copies           the sum of in_flight over the samples (with period 1: the copies the cluster sent)
      died_at          the tick word of the last sample with queued + in_flight > 0 when a later sample exists, else None
      reach_at_death   the reach at that sample, else None
      copies_per_node  copies / reach (None while nobody has been reached)
    headers, records: as Sim.ledger_read returns them."""
    headers, records = np.asarray(headers), np.asarray(records)
    out = []
    for i in range(records.shape[1] if records.ndim == 2 and len(records) else 0):   # (no sample: nothing to say)
        r = records[:, i]
        ticks = headers["tick"].astype(np.int64)
        carried = (r["queued"].astype(np.int64) + r["in_flight"].astype(np.int64)) > 0
        seen = np.nonzero(carried | (r["reach"] > 0))[0]
        last = np.nonzero(carried)[0]
        died = len(last) > 0 and last[-1] + 1 < len(r)
        reach, copies = int(r["reach"][-1]), int(r["in_flight"].astype(np.int64).sum())
        out.append(dict(kind=int(r["id"][0] >> np.uint64(32)), key=int(r["id"][0] & np.uint64(0xFFFFFFFF)), val=int(r["val"][0]),
                        first_tick=int(ticks[seen[0]]) if len(seen) else None,
                        reach=reach, running=int(headers["running"][-1]), copies=copies,
                        died_at=int(ticks[last[-1]]) if died else None,
                        reach_at_death=int(r["reach"][last[-1]]) if died else None,
                        copies_per_node=copies / reach if reach else None))
    return out


# include/serf_sim_detect.h: detection log (per member that owns a view slot: the episodes in which it was down or accused, judged
# behind the sampled ticks).  The sixth extension: a version of its own, bound only when the loaded library exports it
DETECT_SYMBOLS = ("detect_start", "detect_count", "detect_read", "detect_log_count", "detect_log_read", "detect_open", "detect_stop",
                  "detect_version")
DETECT_WORDS, DETECT_EPISODE_WORDS, DETECT_MAX_SAMPLES, DETECT_MAX_LOG, DETECT_NEVER = 64, 8, 1 << 20, 1 << 24, 0xFFFFFFFF
DETECT_DOWN, DETECT_ACCUSED = 1, 2
DETECT_OPEN, DETECT_DETECTED, DETECT_RETURNED, DETECT_CLEARED, DETECT_STOPPED, DETECT_ABANDONED = range(6)
DETECT_F_CENSORED, DETECT_F_AFTER_RETURN = 1, 2
DETECT_OUTCOMES = ("open", "detected", "returned", "cleared", "stopped", "abandoned")
# a sample's header and one episode as numpy records: the tables of include/serf_sim_detect.h, little-endian, the halves of the
# packed words under names of their own ("closed" of a header: by outcome 1 .. 5)
DETECT_HEADER_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("subjects", "<u8"), ("open_down", "<u8"), ("open_accused", "<u8"),
                                ("closed_now", "<u8"), ("log_written", "<u8"), ("log_lost", "<u8"), ("closed", "<u8", (5,)),
                                ("false_declared", "<u8"), ("opened_down", "<u8"), ("opened_accused", "<u8"),
                                ("hist_suspect", "<u8", (16,)), ("hist_all", "<u8", (16,)), ("hist_cleared", "<u8", (16,))])
DETECT_EPISODE_DTYPE = np.dtype([("subject", "<u4"), ("slot", "<u4"), ("kind", "u1"), ("outcome", "u1"), ("flags", "<u2"), ("zero", "<u4"),
                                 ("opened", "<u4"), ("closed", "<u4"), ("first_suspect", "<u4"), ("first_failed", "<u4"),
                                 ("half", "<u4"), ("p99", "<u4"), ("all", "<u4"), ("evaluated", "<u4"), ("peak", "<u8"),
                                 ("peak_susp", "<u8")])
assert DETECT_HEADER_DTYPE.itemsize == 8 * DETECT_WORDS and DETECT_EPISODE_DTYPE.itemsize == 8 * DETECT_EPISODE_WORDS


def detect_bin(x):
    """The histogram bin of a latency x (include/serf_sim_detect.h): x == 0 ? 0 : min(15, 1 + floor(log2 x))."""
    return 0 if x == 0 else min(15, int(x).bit_length())


def detect_summary(episodes):
    """What a detection log says, from its episodes (Sim.detect_log, with or without Sim.detect_open behind them) — a dict
    "<kind>/<outcome>" -> dict(count, censored, and per latency its median, p99 and the number n of episodes that have it):
      suspect   first_suspect - opened     failed   first_failed - opened     half, p99, all   likewise (DOWN episodes)
      length    closed - opened (closed episodes)
    Latencies are taken over the episodes that are not CENSORED (their `opened` is the first sample, not the stop) and that
    latched the tick; count covers all, censored says how many of them are."""
    ep = np.asarray(episodes)
    out = {}
    for kind, kname in ((DETECT_DOWN, "down"), (DETECT_ACCUSED, "accused")):
        for oc, oname in enumerate(DETECT_OUTCOMES):
            sel = ep[(ep["kind"] == kind) & (ep["outcome"] == oc)] if len(ep) else ep
            if not len(sel):
                continue
            cens = (sel["flags"] & DETECT_F_CENSORED) != 0
            d = dict(count=int(len(sel)), censored=int(cens.sum()))
            ok = sel[~cens]
            lat = [("suspect", "first_suspect"), ("failed", "first_failed"), ("length", "closed")]
            if kind == DETECT_DOWN:
                lat += [("half", "half"), ("p99", "p99"), ("all", "all")]
            for name, field in lat:
                x = ok[ok[field] != DETECT_NEVER]
                v = x[field].astype(np.int64) - x["opened"].astype(np.int64)
                d[name] = dict(n=int(len(v)), median=float(np.median(v)) if len(v) else None,
                               p99=float(np.percentile(v, 99)) if len(v) else None)
            out[f"{kname}/{oname}"] = d
    return out


# include/serf_sim_spread.h: spread map (per record identity and node: the tick at which the node first had applied it, latched behind
# the sampled ticks).  The seventh extension: a version of its own, bound only when the loaded library exports it
SPREAD_SYMBOLS = ("spread_start", "spread_count", "spread_read", "spread_stop", "spread_map", "spread_summary", "spread_unreached",
                  "spread_late", "spread_version")
SPREAD_HEADER_WORDS, SPREAD_ENTRY_WORDS, SPREAD_MAX, SPREAD_MAX_SAMPLES = 8, 8, 64, 1 << 20
SPREAD_BINS, SPREAD_SUMMARY_WORDS, SPREAD_TOP_MAX, SPREAD_NODE_WORDS = 32, 40, 64, 8
SPREAD_BY_MISSED, SPREAD_BY_LATE = 0, 1
# a sample's header, one entry's record, one entry's summary and one node's record as numpy records: the tables of
# include/serf_sim_spread.h ("id" of an entry = key | kind << 32; "id" of a node = the node, "running" its flag)
SPREAD_HEADER_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("n", "<u8"), ("new", "<u8"), ("started", "<u8"), ("full", "<u8"),
                                ("reserved", "<u8", (2,))])
SPREAD_ENTRY_DTYPE = np.dtype([("id", "<u8"), ("val", "<u8"), ("new", "<u8"), ("reached", "<u8"), ("reached_up", "<u8"), ("holds", "<u8"),
                               ("first", "<u8"), ("last", "<u8")])
SPREAD_SUMMARY_DTYPE = np.dtype([("id", "<u8"), ("val", "<u8"), ("first", "<u8"), ("last", "<u8"), ("reached", "<u8"), ("reached_up", "<u8"),
                                 ("unreached_up", "<u8"), ("late_sum", "<u8"), ("bins", "<u8", (SPREAD_BINS,))])
SPREAD_NODE_DTYPE = np.dtype([("id", "<u4"), ("running", "<u4"), ("got", "<u8"), ("missed", "<u8"), ("late_sum", "<u8"), ("late_max", "<u8"),
                              ("reserved", "<u8", (3,))])
assert SPREAD_HEADER_DTYPE.itemsize == 8 * SPREAD_HEADER_WORDS and SPREAD_ENTRY_DTYPE.itemsize == 8 * SPREAD_ENTRY_WORDS
assert SPREAD_SUMMARY_DTYPE.itemsize == 8 * SPREAD_SUMMARY_WORDS and SPREAD_NODE_DTYPE.itemsize == 8 * SPREAD_NODE_WORDS


def spread_split(words, n):
    """[samples * (8 + 8 * n)] words -> (headers[samples], records[samples][n])."""
    return sample_split(words, SPREAD_HEADER_DTYPE, SPREAD_ENTRY_DTYPE, n)


def spread_percentiles(map_row, qs):
    """The arrival ticks below which the given shares of the REACHED nodes of one entry lie: for every q of qs (0 < q <= 100)
    the smallest arrival a such that at least q % of the nodes with a non-zero arrival have one <= a (the nearest-rank
    percentile: an integer tick that occurs in the row); None for every q when nobody was reached.  map_row: one entry's
    plane as Sim.spread_map returns it."""
    a = np.sort(np.asarray(map_row, np.int64)[np.asarray(map_row) != 0])
    out = []
    for q in qs:
        if not 0 < q <= 100:
            raise ValueError(f"percentile {q} outside (0, 100]")
        if not len(a):
            out.append(None)
            continue
        rank = -(-int(round(q * 1000)) * len(a) // 100000)          # ceil(q / 100 * len) in integers (q to three decimals)
        out.append(int(a[max(1, rank) - 1]))
    return out


def spread_rank(nodes, rank_by=SPREAD_BY_MISSED, top_k=None):
    """The order sim_spread_late lists the RUNNING nodes in, from every node's record (SPREAD_NODE_DTYPE [n_nodes]):
    SPREAD_BY_MISSED (missed descending, late_sum descending, id ascending), SPREAD_BY_LATE (late_sum descending, missed
    descending, id ascending).  Returns the node ids, the first top_k of them when given."""
    nodes = np.asarray(nodes)
    run = nodes[nodes["running"] != 0]
    missed, late, ids = run["missed"].astype(np.int64), run["late_sum"].astype(np.int64), run["id"].astype(np.int64)
    order = np.lexsort((ids, -late, -missed) if rank_by == SPREAD_BY_MISSED else (ids, -missed, -late))
    return [int(x) for x in ids[order][:top_k]]


# include/serf_sim_traffic.h: traffic meter (per node the gossip packets, records and 16-byte units it sent and had addressed to it,
# accumulated behind the sampled ticks).  The eighth extension: a version of its own, bound only when the loaded library exports it
TRAFFIC_SYMBOLS = ("traffic_start", "traffic_count", "traffic_read", "traffic_stop", "traffic_nodes", "traffic_top", "traffic_summary",
                   "traffic_version")
TRAFFIC_WORDS, TRAFFIC_MAX_SAMPLES, TRAFFIC_COLUMNS, TRAFFIC_TOP_MAX = 64, 1 << 20, 8, 64
TRAFFIC_DEG_BINS, TRAFFIC_REC_BINS, TRAFFIC_BINS, TRAFFIC_SUMMARY_WORDS = 32, 16, 32, 40
TRAFFIC_COLUMN_NAMES = ("tx_packets", "tx_records", "tx_units", "rx_packets", "rx_records", "rx_units", "rx_peak", "rx_down")
TRAFFIC_UNIT_BYTES = 16
# a sample, a node's record, a ranked node and a column's summary as numpy records: the tables of include/serf_sim_traffic.h
TRAFFIC_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("packets", "<u8"), ("records", "<u8"), ("units", "<u8"), ("senders", "<u8"),
                          ("addressed", "<u8"), ("to_down", "<u8"), ("max_packets", "<u8"), ("max_packets_id", "<u8"), ("max_units", "<u8"),
                          ("max_units_id", "<u8"), ("packet_records_max", "<u8"), ("packet_units_max", "<u8"), ("samples", "<u8"),
                          ("reserved", "<u8"), ("degree_bins", "<u8", (TRAFFIC_DEG_BINS,)), ("record_bins", "<u8", (TRAFFIC_REC_BINS,))])
TRAFFIC_NODE_DTYPE = np.dtype([(name, "<u4") for name in TRAFFIC_COLUMN_NAMES])
TRAFFIC_RANK_DTYPE = np.dtype([("id", "<u4"), ("running", "<u4"), ("node", TRAFFIC_NODE_DTYPE)])
TRAFFIC_SUMMARY_DTYPE = np.dtype([("column", "<u8"), ("bin_width", "<u8"), ("sum", "<u8"), ("max", "<u8"), ("max_id", "<u8"), ("min", "<u8"),
                                  ("nonzero", "<u8"), ("samples", "<u8"), ("bins", "<u8", (TRAFFIC_BINS,))])
assert TRAFFIC_DTYPE.itemsize == 8 * TRAFFIC_WORDS and TRAFFIC_NODE_DTYPE.itemsize == 32 and TRAFFIC_RANK_DTYPE.itemsize == 40
assert TRAFFIC_SUMMARY_DTYPE.itemsize == 8 * TRAFFIC_SUMMARY_WORDS


class TrafficNode(C.Structure):
    _fields_ = [("col", C.c_uint32 * TRAFFIC_COLUMNS)]


class TrafficRank(C.Structure):
    _fields_ = [("id", C.c_uint32), ("running", C.c_uint32), ("node", TrafficNode)]


def traffic_rates(nodes, samples, interval_ms=200):
    """Bytes per second every node sent and had addressed to it, from the map (TRAFFIC_NODE_DTYPE [n_nodes], as Sim.traffic_nodes
    returns it) accumulated over `samples` samples, each standing for one gossip interval of interval_ms: a dict with the two
    arrays "tx" and "rx" (float64 [n_nodes]) and, under "tx_stats" / "rx_stats", their median, 99th percentile and max.  With a
    sampling period above 1 the rates are those of the sampled intervals."""
    nodes = np.asarray(nodes)
    seconds = samples * interval_ms / 1000.0
    out = {}
    for side in ("tx", "rx"):
        rate = nodes[side + "_units"].astype(np.float64) * TRAFFIC_UNIT_BYTES / seconds if seconds > 0 else np.zeros(len(nodes))
        out[side] = rate
        out[side + "_stats"] = ({"median": float(np.median(rate)), "p99": float(np.percentile(rate, 99)), "max": float(rate.max())}
                                if len(rate) else {"median": 0.0, "p99": 0.0, "max": 0.0})
    return out


# include/serf_sim_tree.h: rumour tree (per record identity and node: the arrival, the node whose packet brought the rumour, the hop
# count from the origin, latched behind every tick).  The ninth extension: a version of its own, bound only when the loaded library
# exports it
TREE_SYMBOLS = ("tree_start", "tree_count", "tree_read", "tree_stop", "tree_links", "tree_summary", "tree_path", "tree_top", "tree_version")
TREE_HEADER_WORDS, TREE_ENTRY_WORDS, TREE_MAX, TREE_MAX_SAMPLES = 8, 8, 64, 1 << 20
TREE_BINS, TREE_SUMMARY_WORDS, TREE_TOP_MAX, TREE_NONE = 32, 72, 64, 0xFFFFFFFF
# a sample's header, one entry's record, one node's link, a ranked node and one entry's summary as numpy records: the tables of
# include/serf_sim_tree.h ("id" of an entry = key | kind << 32)
TREE_HEADER_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("n", "<u8"), ("new", "<u8"), ("new_orphans", "<u8"), ("copies", "<u8"),
                              ("fresh", "<u8"), ("reserved", "<u8")])
TREE_ENTRY_DTYPE = np.dtype([("id", "<u8"), ("val", "<u8"), ("new", "<u8"), ("new_orphans", "<u8"), ("reached", "<u8"), ("orphans", "<u8"),
                             ("copies", "<u8"), ("fresh", "<u8")])
TREE_LINK_DTYPE = np.dtype([("arrival", "<u4"), ("parent", "<u4"), ("hop", "<u4"), ("children", "<u4")])
TREE_RANK_DTYPE = np.dtype([("id", "<u4"), ("running", "<u4"), ("link", TREE_LINK_DTYPE)])
TREE_SUMMARY_DTYPE = np.dtype([("id", "<u8"), ("val", "<u8"), ("reached", "<u8"), ("orphans", "<u8"), ("depth", "<u8"), ("hop_sum", "<u8"),
                               ("most_children", "<u8"), ("most_children_id", "<u8"), ("hop_bins", "<u8", (TREE_BINS,)),
                               ("children_bins", "<u8", (TREE_BINS,))])
assert TREE_HEADER_DTYPE.itemsize == 8 * TREE_HEADER_WORDS and TREE_ENTRY_DTYPE.itemsize == 8 * TREE_ENTRY_WORDS
assert TREE_LINK_DTYPE.itemsize == 16 and TREE_RANK_DTYPE.itemsize == 24 and TREE_SUMMARY_DTYPE.itemsize == 8 * TREE_SUMMARY_WORDS


class TreeLink(C.Structure):
    _fields_ = [("arrival", C.c_uint32), ("parent", C.c_uint32), ("hop", C.c_uint32), ("children", C.c_uint32)]


class TreeRank(C.Structure):
    _fields_ = [("id", C.c_uint32), ("running", C.c_uint32), ("link", TreeLink)]


def tree_split(words, n):
    """[samples * (8 + 8 * n)] words -> (headers[samples], records[samples][n])."""
    return sample_split(words, TREE_HEADER_DTYPE, TREE_ENTRY_DTYPE, n)


def tree_hops(links, qs=(50, 90, 99, 100)):
    """The hop-count percentiles and the share of orphans of one entry's tree, from every node's link (TREE_LINK_DTYPE, as
    Sim.tree_links returns them): a dict with "reached", "orphans", "orphan_share" (orphans / reached, 0.0 when nobody is
    reached), "depth", "mean_hop" and "percentiles" — for every q of qs (0 < q <= 100) the smallest hop h such that at least
    q % of the reached nodes have one <= h (the nearest-rank percentile: a hop count that occurs), None when nobody is reached."""
    links = np.asarray(links)
    got = links[links["arrival"] != 0]
    hop = np.sort(got["hop"].astype(np.int64))
    pct = {}
    for q in qs:
        if not 0 < q <= 100:
            raise ValueError(f"percentile {q} outside (0, 100]")
        rank = -(-int(round(q * 1000)) * len(hop) // 100000)            # ceil(q / 100 * len) in integers (q to three decimals)
        pct[q] = int(hop[max(1, rank) - 1]) if len(hop) else None
    orphans = int((got["parent"] == TREE_NONE).sum())
    return {"reached": len(got), "orphans": orphans, "orphan_share": orphans / len(got) if len(got) else 0.0,
            "depth": int(hop[-1]) if len(hop) else 0, "mean_hop": float(hop.mean()) if len(hop) else 0.0, "percentiles": pct}


class LedgerEntry(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("key", C.c_uint32), ("val", C.c_uint64)]


# include/serf_sim_qboard.h: query board (per followed query id: acks, responses, who of the eligible nodes answered, who stayed
# silent, the 50 / 90 / 99 / 100 % latches, sampled behind the ticks).  The tenth extension: a version of its own, bound only when
# the loaded library exports it
QBOARD_SYMBOLS = ("qboard_start", "qboard_count", "qboard_read", "qboard_stop", "qboard_now", "qboard_silent", "qboard_nodes", "qboard_top",
                  "qboard_version")
QBOARD_HEADER_WORDS, QBOARD_ENTRY_WORDS, QBOARD_MAX, QBOARD_MAX_SAMPLES = 8, 16, 64, 1 << 20
QBOARD_TOP_MAX, QBOARD_NODE_WORDS = 64, 8
QBOARD_WAITING, QBOARD_OPEN, QBOARD_CLOSED, QBOARD_DISPLACED = 0, 1, 2, 3
QBOARD_BY_SILENT_ACK, QBOARD_BY_SILENT_RESP = 0, 1
# a sample's header, one entry's record and one node's record as numpy records: the tables of include/serf_sim_qboard.h
QBOARD_HEADER_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("n", "<u8"), ("open", "<u8"), ("closed", "<u8"), ("waiting", "<u8"),
                                ("displaced", "<u8"), ("new", "<u8")])
QBOARD_ENTRY_DTYPE = np.dtype([("id", "<u4"), ("state", "<u4"), ("origin", "<u4"), ("flags", "<u4"), ("deadline", "<u8"), ("acks", "<u8"),
                               ("responses", "<u8"), ("eligible", "<u8"), ("answered", "<u8"), ("responded", "<u8"), ("silent", "<u8"),
                               ("new_acks", "<u8"), ("new_responses", "<u8"), ("t_first", "<u8"), ("t_half", "<u8"), ("t_90", "<u8"),
                               ("t_99", "<u8"), ("t_all", "<u8")])
QBOARD_NODE_DTYPE = np.dtype([("id", "<u4"), ("running", "<u4"), ("asked", "<u8"), ("acked", "<u8"), ("responded", "<u8"), ("silent_ack", "<u8"),
                              ("silent_resp", "<u8"), ("reserved", "<u8", (2,))])
QBOARD_SUMMARY_DTYPE = np.dtype([("id", "<u4"), ("state", "<u4"), ("started", "<i8"), ("deadline", "<i8"), ("acks", "<i8"), ("responses", "<i8"),
                                 ("answered", "<i8"), ("eligible", "<i8"), ("to_half", "<i8"), ("to_90", "<i8"), ("to_99", "<i8"),
                                 ("to_all", "<i8"), ("silent_at_close", "<i8")])
assert QBOARD_HEADER_DTYPE.itemsize == 8 * QBOARD_HEADER_WORDS and QBOARD_ENTRY_DTYPE.itemsize == 8 * QBOARD_ENTRY_WORDS
assert QBOARD_NODE_DTYPE.itemsize == 8 * QBOARD_NODE_WORDS


def qboard_split(words, n):
    """[samples * (8 + 16 * n)] words -> (headers[samples], records[samples][n])."""
    return sample_split(words, QBOARD_HEADER_DTYPE, QBOARD_ENTRY_DTYPE, n)


def qboard_rank(nodes, rank_by=QBOARD_BY_SILENT_ACK, top_k=None):
    """The order sim_qboard_top lists the RUNNING nodes in, from every node's record (QBOARD_NODE_DTYPE [n_nodes]): silent_ack
    (QBOARD_BY_SILENT_ACK) or silent_resp (QBOARD_BY_SILENT_RESP) descending, id ascending.  Returns the node ids, the first
    top_k of them when given."""
    nodes = np.asarray(nodes)
    run = nodes[nodes["running"] != 0]
    score = run["silent_ack" if rank_by == QBOARD_BY_SILENT_ACK else "silent_resp"].astype(np.int64)
    ids = run["id"].astype(np.int64)
    return [int(x) for x in ids[np.lexsort((ids, -score))][:top_k]]


def qboard_summary(records, q_timeout):
    """One row per query (QBOARD_SUMMARY_DTYPE [entries]) from the records of a board's samples (QBOARD_ENTRY_DTYPE [samples][entries],
    as Sim.qboard_read returns them); q_timeout: the query timeout in ticks (16 per decimal digit of n_nodes).  Per entry, over its
    LAST run (the samples since the table entry last changed hands or started afresh): `started` = deadline - q_timeout, the
    deadline, the final acks and responses (of the last sample that was open or closed), answered / eligible at the last OPEN
    sample, the ticks from `started` to the half / 90 / 99 / all latches (-1: never latched) and `silent_at_close` = silent at the
    first closed sample (-1: never seen closed).  An entry that never left `waiting` has state 0 and -1 in every other column."""
    records = np.asarray(records)
    out = np.zeros(records.shape[1] if records.ndim == 2 else 0, QBOARD_SUMMARY_DTYPE)
    for name in out.dtype.names[2:]:
        out[name] = -1
    for i in range(len(out)):
        col = records[:, i]
        out["id"][i] = col["id"][0] if len(col) else 0
        live = np.nonzero((col["state"] == QBOARD_OPEN) | (col["state"] == QBOARD_CLOSED))[0]
        if not len(live):
            continue
        last = col[live[-1]]
        run = [k for k in live.tolist() if col["deadline"][k] == last["deadline"] and col["origin"][k] == last["origin"] and col["flags"][k] == last["flags"]]
        row = out[i]
        row["state"] = col["state"][-1]
        row["deadline"], row["started"] = int(last["deadline"]), int(last["deadline"]) - q_timeout
        row["acks"], row["responses"] = int(last["acks"]), int(last["responses"])
        opened = [k for k in run if col["state"][k] == QBOARD_OPEN]
        if opened:
            row["answered"], row["eligible"] = int(col["answered"][opened[-1]]), int(col["eligible"][opened[-1]])
        for name, latch in (("to_half", "t_half"), ("to_90", "t_90"), ("to_99", "t_99"), ("to_all", "t_all")):
            if last[latch]:
                row[name] = int(last[latch]) - int(row["started"])
        closed = [k for k in run if col["state"][k] == QBOARD_CLOSED]
        if closed:
            row["silent_at_close"] = int(col["silent"][closed[0]])
    return out


# include/serf_sim_catalog.h: rumour catalogue (the live record identities FOUND behind the ticks, not named in advance, and a
# registry of every identity ever found).  The eleventh extension: a version of its own, bound only when the loaded library
# exports it
CATALOG_SYMBOLS = ("catalog_start", "catalog_count", "catalog_read", "catalog_stop", "catalog_list", "catalog_live", "catalog_now",
                   "catalog_version")
CATALOG_LIVE, CATALOG_MAX, CATALOG_MAX_SAMPLES, CATALOG_SAMPLE_WORDS, CATALOG_RECORD_WORDS, CATALOG_KINDS = 256, 4096, 1 << 20, 48, 8, 0xFE
# a sample, a live identity (the ledger's entry layout) and a registry record as numpy records: the tables of
# include/serf_sim_catalog.h.  by-kind columns: index 0 is kind 1
CATALOG_SAMPLE_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("live", "<u8"), ("overflow", "<u8"), ("new", "<u8"), ("died", "<u8"),
                                 ("revived", "<u8"), ("registry", "<u8"), ("ids_lost", "<u8"), ("queued", "<u8"), ("in_flight", "<u8"),
                                 ("packets", "<u8"), ("transmits", "<u8"), ("live_by_kind", "<u8", (7,)), ("queued_by_kind", "<u8", (7,)),
                                 ("in_flight_by_kind", "<u8", (7,)), ("overflowed", "<u8"), ("reserved", "<u8", (13,))])
CATALOG_LIVE_DTYPE = np.dtype([("id", "<u8"), ("val", "<u8"), ("reserved", "<u8"), ("holders", "<u8"), ("queued", "<u8"),
                               ("transmits", "<u8"), ("in_flight", "<u8"), ("fresh", "<u8")])
CATALOG_RECORD_DTYPE = np.dtype([("id", "<u8"), ("val", "<u8"), ("first_seen", "<u4"), ("last_seen", "<u4"), ("samples", "<u4"),
                                 ("revivals", "<u4"), ("peak_queued", "<u4"), ("peak_queued_at", "<u4"), ("peak_holders", "<u4"),
                                 ("peak_holders_at", "<u4"), ("in_flight_sum", "<u8"), ("queued_sum", "<u8")])
assert CATALOG_SAMPLE_DTYPE.itemsize == 8 * CATALOG_SAMPLE_WORDS
assert CATALOG_LIVE_DTYPE.itemsize == CATALOG_RECORD_DTYPE.itemsize == 8 * CATALOG_RECORD_WORDS


def catalog_mask(kinds):
    """Kinds (1-7) -> kinds_mask: bit k set means kind k is catalogued."""
    m = 0
    for k in kinds:
        m |= 1 << int(k)
    return m


def catalog_summary(records):
    """What a catalogue's registry (CATALOG_RECORD_DTYPE, as Sim.catalog_list returns it) says, as a dict: `identities` — one
    dict per record, in the registry's order, with kind, key, val and the record's fields —, and `by_kind`: kind -> how many
    identities the registry holds of it, the copies sent for them (in_flight_sum) and the longest life in ticks."""
    records = np.asarray(records)
    ids, by_kind = [], {}
    for r in records:
        kind, key = int(r["id"]) >> 32, int(r["id"]) & 0xFFFFFFFF
        d = dict(kind=kind, key=key, val=int(r["val"]))
        d.update({n: int(r[n]) for n in CATALOG_RECORD_DTYPE.names[2:]})
        ids.append(d)
        k = by_kind.setdefault(kind, dict(identities=0, copies=0, longest_life=0))
        k["identities"] += 1
        k["copies"] += d["in_flight_sum"]
        k["longest_life"] = max(k["longest_life"], d["last_seen"] - d["first_seen"] + 1)
    return dict(identities=ids, by_kind=dict(sorted(by_kind.items())))


# include/serf_sim_gazette.h: member gazette (every node's member events — Join / Leave / Failed / Reap, flaps — by view
# diffs behind the ticks, per node and per subject).  The twelfth extension: a version of its own, bound only when the
# loaded library exports it
GAZETTE_SYMBOLS = ("gazette_start", "gazette_count", "gazette_read", "gazette_nodes", "gazette_subjects", "gazette_top", "gazette_stop",
                   "gazette_version")
GAZETTE_WORDS, GAZETTE_COLS, GAZETTE_TOP_MAX, GAZETTE_MAX_SAMPLES = 64, 8, 64, 1 << 20
GAZETTE_MAP_NODES, GAZETTE_MAP_SUBJECTS = 0, 1
GAZETTE_COLUMNS = ("join", "leave", "failed", "reap", "flap", "suspected", "cleared", "peak")
GAZETTE_JOIN, GAZETTE_LEAVE, GAZETTE_FAILED, GAZETTE_REAP, GAZETTE_FLAP, GAZETTE_SUSPECTED, GAZETTE_CLEARED, GAZETTE_PEAK = range(8)
# a sample and a place of a ranking as numpy records: the tables of include/serf_sim_gazette.h
GAZETTE_SAMPLE_DTYPE = np.dtype([("tick", "<u8"), ("running", "<u8"), ("slots", "<u8"), ("fresh", "<u8"), ("matrix", "<u8", (5, 5)),
                                 ("swim", "<u8", (4, 4)), ("sums", "<u8", (7,)), ("nodes", "<u8"), ("node_max", "<u8"), ("node_id", "<u8"),
                                 ("subjects", "<u8"), ("subject_id", "<u8"), ("subject_max", "<u8"), ("dead_time", "<u8", (5,)),
                                 ("reserved", "<u8")])
GAZETTE_RANK_DTYPE = np.dtype([("id", "<u8"), ("row", "<u4", (8,))])
assert GAZETTE_SAMPLE_DTYPE.itemsize == 8 * GAZETTE_WORDS and GAZETTE_RANK_DTYPE.itemsize == 40


def gazette_rates(samples, nodes=None):
    """What a gazette's samples (GAZETTE_SAMPLE_DTYPE, as Sim.gazette_read returns them) say, as a dict: the ticks they span,
    per column 0-6 the total and the events per tick — serf.member.join / leave / flap among them —, and with `nodes` (the
    node map, as Sim.gazette_nodes returns it) the median, the 99th percentile and the maximum of the events of columns 0-3 a
    node saw."""
    samples = np.asarray(samples)
    out = dict(samples=int(len(samples)), ticks=0, totals={}, per_tick={})
    if len(samples):
        out["ticks"] = int(samples["tick"][-1]) - int(samples["tick"][0]) + 1
    sums = samples["sums"].astype(np.int64).sum(axis=0) if len(samples) else np.zeros(7, np.int64)
    for k, name in enumerate(GAZETTE_COLUMNS[:7]):
        out["totals"][name] = int(sums[k])
        out["per_tick"][name] = float(sums[k]) / out["ticks"] if out["ticks"] else 0.0
    if nodes is not None:
        ev = np.asarray(nodes)[:, :4].astype(np.int64).sum(axis=1)
        srt = np.sort(ev)
        pick = lambda q: int(srt[min(len(srt) - 1, int(np.ceil(q * len(srt))) - 1)]) if len(srt) else 0     # nearest rank
        out["per_node"] = dict(median=pick(0.5), p99=pick(0.99), max=int(srt[-1]) if len(srt) else 0)
    return out


class SpreadEntry(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("key", C.c_uint32), ("ltime", C.c_uint64)]


def spread_entries(entries):
    """(kind, key, ltime) triples (or SpreadEntry) -> a ctypes array of SpreadEntry."""
    es = [e if isinstance(e, SpreadEntry) else SpreadEntry(int(e[0]), int(e[1]), int(e[2])) for e in entries]
    return (SpreadEntry * max(1, len(es)))(*es)


def ledger_entries(entries):
    """(kind, key, val) triples (or LedgerEntry) -> a ctypes array of LedgerEntry."""
    es = [e if isinstance(e, LedgerEntry) else LedgerEntry(int(e[0]), int(e[1]), int(e[2])) for e in entries]
    return (LedgerEntry * max(1, len(es)))(*es)


class Tracker(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32), ("min_inc", C.c_uint32),
                ("ltime", C.c_uint64), ("start_tick", C.c_uint32), ("max_age", C.c_uint32)]


class TrackResult(C.Structure):
    _fields_ = [("first", C.c_uint32), ("half", C.c_uint32), ("p90", C.c_uint32), ("p99", C.c_uint32), ("all", C.c_uint32),
                ("evaluated", C.c_uint32), ("peak", C.c_uint64), ("last", C.c_uint64), ("last_up", C.c_uint64),
                ("state", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "pad"}


def make_config(n_nodes, *, fanout=3, vshards=1, shard_rank=0, shard_count=1, view_slots=0,
                event_ring=512, query_ring=512, retransmit_mult=4, probe_interval=0,
                suspicion_mult=4, suspicion_max_mult=6, indirect_checks=3, loss=0.0,
                intent_timeout=0, leave_delay=30, reap_interval=0, reconnect_timeout=432000, tombstone_timeout=432000,
                queue_check_interval=0, max_queue_depth=4096, min_queue_depth=0, push_pull_interval=0, chunks=0, recycle_interval=0,
                pkt_records=0, gossip_to_the_dead=0, reconnect_interval=0, ring_overflow=0, tcp_fallback=False, nacks=False, awareness_probe=False, join_sync=False, force_sharded=False, prune_delay=False, flags=CF_BASELINE_JOINED, seed=DEFAULT_SEED):
    cfg = Config()
    cfg.struct_size = C.sizeof(Config)
    cfg.n_nodes, cfg.vshards, cfg.shard_rank, cfg.shard_count = n_nodes, vshards, shard_rank, shard_count
    cfg.fanout, cfg.view_slots, cfg.event_ring, cfg.query_ring = fanout, view_slots, event_ring, query_ring
    cfg.retransmit_mult, cfg.probe_interval = retransmit_mult, probe_interval
    cfg.suspicion_mult, cfg.suspicion_max_mult, cfg.indirect_checks = suspicion_mult, suspicion_max_mult, indirect_checks
    cfg.loss_u32 = min(0xFFFFFFFF, int(round(loss * 2 ** 32)))
    cfg.intent_timeout, cfg.leave_delay, cfg.flags, cfg.seed = intent_timeout, leave_delay, flags, seed
    cfg.reap_interval, cfg.reconnect_timeout, cfg.tombstone_timeout = reap_interval, reconnect_timeout, tombstone_timeout
    cfg.queue_check_interval, cfg.max_queue_depth, cfg.min_queue_depth = queue_check_interval, max_queue_depth, min_queue_depth
    cfg.push_pull_interval, cfg.chunks, cfg.recycle_interval = push_pull_interval, chunks, recycle_interval
    cfg.pkt_records = pkt_records  # 0 = 4 records (one page) per packet; 8 / 12 / 16 = more pages
    cfg.gossip_to_the_dead = gossip_to_the_dead
    cfg.reconnect_interval = reconnect_interval  # Reconnector (base.rs:612-681): 0 = off
    cfg.ring_overflow = ring_overflow  # overflow rows per de-dup ring and node (a full bucket's further keys); 0 = none
    if awareness_probe:
        cfg.flags |= CF_AWARENESS_PROBE
    if join_sync:
        cfg.flags |= CF_JOIN_SYNC
    if tcp_fallback:
        cfg.flags |= CF_TCP_FALLBACK   # memberlist's stream-transport fallback ping: packet loss alone never fails a probe
    if nacks:
        cfg.flags |= CF_NACKS          # awareness += relays that were asked and did not nack
    if force_sharded:
        cfg.flags |= CF_FORCE_SHARDED  # one rank of the N > 1 path: exchange buffers, the sharded kernel, host-driven push-pull
    if prune_delay:
        cfg.flags |= CF_PRUNE_DELAY    # handle_prune's wait (base.rs:1628-1653): a Leaving member's forced erase comes leave_delay ticks later
    return cfg


def rumour_tracker(kind, key, ltime, start=0, max_age=0):
    return Tracker(TRK_RUMOUR, kind, key, 0, ltime, start, max_age)


def member_tracker(subject, status_mask, swim_mask=0, min_inc=0, start=0, max_age=0):
    return Tracker(TRK_MEMBER, subject, (status_mask & 0xFF) | (swim_mask << 8), min_inc, 0, start, max_age)


class SimLib:
    """One loaded implementation of the ABI."""

    def __init__(self, path, prefix="sim_", optional=()):
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"{path} is missing — build it first (python -c 'import __graft_entry__ as g; g.build()')")
        self.path, self.prefix = path, prefix
        self.dll = C.CDLL(path)
        self.f = {}
        H, u32, u64, vp = C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p
        sig = {
            "create": (C.c_int, [C.POINTER(Config), C.POINTER(H)]),
            "destroy": (C.c_int, [H]),
            "set_stream": (C.c_int, [H, vp]),
            "join": (C.c_int, [H, u32, u32]),
            "leave": (C.c_int, [H, u32]),
            "force_leave": (C.c_int, [H, u32, u32, C.c_int]),
            "user_event": (C.c_int, [H, u32, u32, u32, C.c_int]),
            "query": (C.c_int, [H, u32, u32, u32]),
            "query_filtered": (C.c_int, [H, u32, u32, u32, C.POINTER(u32), u32, u32]),
            "set_tags": (C.c_int, [H, u32, u32]),
            "init_tags": (C.c_int, [H, u32, u32, vp]),
            "inject": (C.c_int, [H, u64, u32, u32, u32, u32]),
            "step": (C.c_int, [H, u32]),
            "sync": (C.c_int, [H]),
            "tick": (C.c_int, [H, C.POINTER(u64)]),
            "members": (C.c_int, [H, u32, vp, vp, u32]),
            "stats_get": (C.c_int, [H, u32, C.POINTER(Stats)]),
            "watch": (C.c_int, [H, u32]),
            "drain_events": (C.c_int, [H, C.POINTER(Event), u32, C.POINTER(u32)]),
            "state_digest": (C.c_int, [H, C.POINTER(u64 * 8)]),
            "dump_state": (C.c_int, [H, u32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "convergence": (C.c_int, [H, u32, u32, u64, C.POINTER(u64), C.POINTER(u64)]),
            "convergence_many": (C.c_int, [H, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
            "exchange_bytes": (C.c_int, [H, C.POINTER(C.c_size_t)]),
            "bind_exchange": (C.c_int, [H, vp, vp]),
            "bind_exchange2": (C.c_int, [H, vp, vp, vp]),
            "bind_exchange3": (C.c_int, [H, vp, C.c_size_t, vp, vp, C.c_size_t]),
            "exchange_chunks": (C.c_int, [H, C.POINTER(u32), C.POINTER(C.c_size_t)]),
            "exchange_layout": (C.c_int, [H, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
            "resident_planes": (C.c_int, [H, C.POINTER(u32), C.POINTER(C.c_uint64)]),
            "step_begin": (C.c_int, [H]),
            "step_chunk": (C.c_int, [H, u32]),
            "step_end": (C.c_int, [H]),
            "pp_due": (C.c_int, [H]),
            "pp_plan": (C.c_int, [H, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_size_t)]),
            "pp_export": (C.c_int, [H, C.c_int, vp]),
            "pp_merge": (C.c_int, [H, C.c_int, vp]),
            "recycle_due": (C.c_int, [H]),
            "recycle_scan": (C.c_int, [H, C.POINTER(RecycleCand), u32, C.POINTER(u32)]),
            "recycle_apply": (C.c_int, [H, C.POINTER(RecycleCand), u32]),
            "snapshot": (C.c_int, [H, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "restore": (C.c_int, [H, vp, C.c_size_t]),
            "query_status": (C.c_int, [H, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int)]),
            "query_responders": (C.c_int, [H, u32, C.c_int, C.POINTER(u32), u32, C.POINTER(u32)]),
            "profile": (C.c_int, [H, C.c_int]),
            "profile_read": (C.c_int, [H, C.POINTER(C.c_double), C.POINTER(u64)]),
            "profile_read_stats": (C.c_int, [H, C.POINTER(C.c_double * 3), C.POINTER(u64)]),
            "cluster_stats_get": (C.c_int, [H, C.POINTER(ClusterStats)]),
            "inject_record": (C.c_int, [H, u64, u32, vp]),
            "deliver_message": (C.c_int, [H, u32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
            "user_event_bytes": (C.c_int, [H, u32, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]),
            "peek_packet": (C.c_int, [H, u32, u32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
            "suspect_requests": (C.c_int, [H, vp, u32, C.POINTER(u32)]),
            "suspect_export": (C.c_int, [H, vp]),
            "suspect_import": (C.c_int, [H, u64, vp, u32]),
            "exchange_unique_id": (C.c_int, [vp]),
            "exchange_init": (C.c_int, [H, vp, u32, u32]),
            "exchange_chunk": (C.c_int, [H, u32]),
            "exchange_wait": (C.c_int, [H]),
            "exchange_library": (C.c_int, [C.c_char_p, C.c_size_t]),
            "abi_version": (u32, []),
            "backend_name": (C.c_char_p, []),
        }
        for name, (res, args) in sig.items():
            if name in optional and not hasattr(self.dll, prefix + name):
                continue   # (tools/ab.py: a build of an older ABI next to the current one)
            fn = getattr(self.dll, prefix + name)  # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
            self.f[name] = fn
        # the twelve extensions: (group, the attribute that says whether the library exports it, symbol -> (restype, argtypes)); a group is
        # bound whole or not at all
        count = (C.c_int, [H, C.POINTER(u32), C.POINTER(u32)])
        read = (C.c_int, [H, u32, u32, vp, C.c_size_t, C.POINTER(u32)])
        stop = (C.c_int, [H])
        ext = [
            ("track", "has_trackers", {
                "track_add": (C.c_int, [H, C.POINTER(Tracker), u32, C.POINTER(u32)]),
                "track_remove": (C.c_int, [H, C.POINTER(u32), u32]),
                "track_read": (C.c_int, [H, C.POINTER(u32), u32, C.POINTER(TrackResult)]),
                "track_active": (C.c_int, [H, C.POINTER(u32), C.POINTER(u32)]),
                "track_version": (u32, []),
            }),
            ("series", "has_series", {
                "series_start": (C.c_int, [H, u32, u32, u32]),
                "series_count": count,
                "series_read": (C.c_int, [H, u32, u32, vp, C.POINTER(u32)]),
                "series_stop": stop,
                "series_version": (u32, []),
            }),
            ("census", "has_census", {
                "census_start": (C.c_int, [H, u32, u32, u32, u32]),
                "census_count": count,
                "census_read": read,
                "census_stop": stop,
                "census_now": (C.c_int, [H, vp, vp, u32, C.POINTER(u32)]),
                "census_version": (u32, []),
            }),
            ("roll", "has_roll", {
                "roll_start": (C.c_int, [H, u32, u32, u32, u32, u32]),
                "roll_count": count,
                "roll_read": read,
                "roll_stop": stop,
                "roll_now": (C.c_int, [H, u32, u32, vp, vp, vp]),
                "roll_version": (u32, []),
            }),
            ("ledger", "has_ledger", {
                "ledger_start": (C.c_int, [H, C.POINTER(LedgerEntry), u32, u32, u32, u32]),
                "ledger_count": count,
                "ledger_read": read,
                "ledger_stop": stop,
                "ledger_now": (C.c_int, [H, C.POINTER(LedgerEntry), u32, vp]),
                "ledger_version": (u32, []),
            }),
            ("detect", "has_detect", {
                "detect_start": (C.c_int, [H, u32, u32, u32, u32]),
                "detect_count": count,
                "detect_read": read,
                "detect_log_count": (C.c_int, [H, C.POINTER(u64), C.POINTER(u64)]),
                "detect_log_read": (C.c_int, [H, u64, u32, vp, u32, C.POINTER(u32)]),
                "detect_open": (C.c_int, [H, vp, u32, C.POINTER(u32)]),
                "detect_stop": stop,
                "detect_version": (u32, []),
            }),
            ("spread", "has_spread", {
                "spread_start": (C.c_int, [H, C.POINTER(SpreadEntry), u32, u32, u32, u32]),
                "spread_count": count,
                "spread_read": read,
                "spread_stop": stop,
                "spread_map": (C.c_int, [H, u32, u32, u32, vp]),
                "spread_summary": (C.c_int, [H, u32, vp]),
                "spread_unreached": (C.c_int, [H, u32, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
                "spread_late": (C.c_int, [H, u32, u32, vp, vp]),
                "spread_version": (u32, []),
            }),
            ("traffic", "has_traffic", {
                "traffic_start": (C.c_int, [H, u32, u32, u32]),
                "traffic_count": count,
                "traffic_read": read,
                "traffic_stop": stop,
                "traffic_nodes": (C.c_int, [H, u32, u32, vp]),
                "traffic_top": (C.c_int, [H, u32, u32, vp]),
                "traffic_summary": (C.c_int, [H, u32, u32, vp]),
                "traffic_version": (u32, []),
            }),
            ("tree", "has_tree", {
                "tree_start": (C.c_int, [H, C.POINTER(SpreadEntry), u32, u32, u32]),
                "tree_count": count,
                "tree_read": read,
                "tree_stop": stop,
                "tree_links": (C.c_int, [H, u32, u32, u32, vp]),
                "tree_summary": (C.c_int, [H, vp]),
                "tree_path": (C.c_int, [H, u32, u32, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
                "tree_top": (C.c_int, [H, u32, u32, vp]),
                "tree_version": (u32, []),
            }),
            ("qboard", "has_qboard", {
                "qboard_start": (C.c_int, [H, C.POINTER(u32), u32, u32, u32, u32]),
                "qboard_count": count,
                "qboard_read": read,
                "qboard_stop": stop,
                "qboard_now": (C.c_int, [H, C.POINTER(u32), u32, vp]),
                "qboard_silent": (C.c_int, [H, u32, u32, vp, u32, C.POINTER(u32), C.POINTER(u32)]),
                "qboard_nodes": (C.c_int, [H, u32, u32, vp]),
                "qboard_top": (C.c_int, [H, u32, u32, vp, vp]),
                "qboard_version": (u32, []),
            }),
            ("catalog", "has_catalog", {
                "catalog_start": (C.c_int, [H, u32, u32, u32, u32, u32]),
                "catalog_count": count,
                "catalog_read": read,
                "catalog_stop": stop,
                "catalog_list": (C.c_int, [H, u32, u32, vp, C.c_size_t, C.POINTER(u32), C.POINTER(u32)]),
                "catalog_live": (C.c_int, [H, vp, C.c_size_t, C.POINTER(u32)]),
                "catalog_now": (C.c_int, [H, u32, vp, vp, C.c_size_t, C.POINTER(u32)]),
                "catalog_version": (u32, []),
            }),
            ("gazette", "has_gazette", {
                "gazette_start": (C.c_int, [H, u32, u32, u32, u32]),
                "gazette_count": count,
                "gazette_read": read,
                "gazette_nodes": (C.c_int, [H, u32, u32, vp]),
                "gazette_subjects": (C.c_int, [H, u32, u32, vp]),
                "gazette_top": (C.c_int, [H, u32, u32, u32, vp]),
                "gazette_stop": stop,
                "gazette_version": (u32, []),
            }),
        ]
        assert [tuple(sigs) for _, _, sigs in ext] == [TRACK_SYMBOLS, SERIES_SYMBOLS, CENSUS_SYMBOLS, ROLL_SYMBOLS, LEDGER_SYMBOLS,
                                                           DETECT_SYMBOLS, SPREAD_SYMBOLS, TRAFFIC_SYMBOLS, TREE_SYMBOLS, QBOARD_SYMBOLS,
                                                           CATALOG_SYMBOLS, GAZETTE_SYMBOLS]
        self.ext = {}   # group -> exported
        for group, attr, sigs in ext:
            self.ext[group] = all(hasattr(self.dll, prefix + name) for name in sigs)
            setattr(self, attr, self.ext[group])
            for name, (res, args) in sigs.items() if self.ext[group] else ():
                fn = getattr(self.dll, prefix + name)
                fn.restype, fn.argtypes = res, args
                self.f[name] = fn

    def backend_name(self):
        return self.f["backend_name"]().decode()

    def exchange_unique_id(self) -> bytes:
        """ncclGetUniqueId through the library (rank 0); the bytes go to every rank, then Sim.exchange_init."""
        buf = C.create_string_buffer(EXCHANGE_ID_BYTES)
        rc = self.f["exchange_unique_id"](buf)
        if rc:
            raise SimError(rc, "sim_exchange_unique_id")
        return buf.raw

    def exchange_library(self):
        """"RCCL x.y.z" of the collective library behind sim_exchange_* (None: the implementation has none)."""
        buf = C.create_string_buffer(64)
        return buf.value.decode() if self.f["exchange_library"](buf, 64) == 0 else None

    def abi_version(self):
        return self.f["abi_version"]()

    def track_version(self):
        """SIM_TRACK_VERSION of include/serf_sim_track.h, or None when the library has no trackers."""
        return self.f["track_version"]() if self.has_trackers else None

    def series_version(self):
        """SIM_SERIES_VERSION of include/serf_sim_series.h, or None when the library has no series."""
        return self.f["series_version"]() if self.has_series else None

    def census_version(self):
        """SIM_CENSUS_VERSION of include/serf_sim_census.h, or None when the library has no census."""
        return self.f["census_version"]() if self.has_census else None

    def roll_version(self):
        """SIM_ROLL_VERSION of include/serf_sim_roll.h, or None when the library has no roll."""
        return self.f["roll_version"]() if self.has_roll else None

    def ledger_version(self):
        """SIM_LEDGER_VERSION of include/serf_sim_ledger.h, or None when the library has no ledger."""
        return self.f["ledger_version"]() if self.has_ledger else None

    def detect_version(self):
        """SIM_DETECT_VERSION of include/serf_sim_detect.h, or None when the library has no detection log."""
        return self.f["detect_version"]() if self.has_detect else None

    def spread_version(self):
        """SIM_SPREAD_VERSION of include/serf_sim_spread.h, or None when the library has no spread map."""
        return self.f["spread_version"]() if self.has_spread else None

    def traffic_version(self):
        """SIM_TRAFFIC_VERSION of include/serf_sim_traffic.h, or None when the library has no traffic meter."""
        return self.f["traffic_version"]() if self.has_traffic else None

    def tree_version(self):
        """SIM_TREE_VERSION of include/serf_sim_tree.h, or None when the library has no rumour tree."""
        return self.f["tree_version"]() if self.has_tree else None

    def qboard_version(self):
        """SIM_QBOARD_VERSION of include/serf_sim_qboard.h, or None when the library has no query board."""
        return self.f["qboard_version"]() if self.has_qboard else None

    def catalog_version(self):
        """SIM_CATALOG_VERSION of include/serf_sim_catalog.h, or None when the library has no rumour catalogue."""
        return self.f["catalog_version"]() if self.has_catalog else None

    def gazette_version(self):
        """SIM_GAZETTE_VERSION of include/serf_sim_gazette.h, or None when the library has no member gazette."""
        return self.f["gazette_version"]() if self.has_gazette else None


class Sim:
    """A simulated cluster behind the C ABI; method names follow ``Serf`` (serf/api.rs)."""

    def __init__(self, lib: SimLib, cfg: Config):
        self.lib, self.cfg = lib, cfg
        self.h = C.c_void_p()
        rc = lib.f["create"](C.byref(cfg), C.byref(self.h))
        if rc:
            self.h = None
            raise SimError(rc, "sim_create")
        self.n = cfg.n_nodes

    def _ck(self, rc, what):
        if rc < 0:
            raise SimError(rc, what)
        return rc

    def close(self):
        if self.h:
            self.lib.f["destroy"](self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- Serf API (api.rs) ----
    def join(self, node, peer=0):
        self._ck(self.lib.f["join"](self.h, node, peer), "sim_join")

    def leave(self, node):
        self._ck(self.lib.f["leave"](self.h, node), "sim_leave")

    def remove_failed_node(self, node, subject, prune=False):
        self._ck(self.lib.f["force_leave"](self.h, node, subject, int(prune)), "sim_force_leave")

    def user_event(self, node, key, encoded_len=32, coalesce=False):
        self._ck(self.lib.f["user_event"](self.h, node, key, encoded_len, int(coalesce)), "sim_user_event")

    def query(self, node, query_id, flags=0, ids=None, tag_mask=NO_TAG_FILTER):
        """Serf::query (api.rs:304).  ids / tag_mask = QueryParam.filters in the form the ABI takes them
        (serf_amd.filters.TagTable.compile turns Filter::Id / Filter::Tag lists into this pair)."""
        if ids is None and tag_mask == NO_TAG_FILTER:
            self._ck(self.lib.f["query"](self.h, node, query_id, flags), "sim_query")
            return
        ids = list(ids or [])
        arr = (C.c_uint32 * max(1, len(ids)))(*ids)
        self._ck(self.lib.f["query_filtered"](self.h, node, query_id, flags, arr, len(ids), tag_mask), "sim_query_filtered")

    def set_tags(self, node, tag_class):
        """Serf::set_tags (api.rs:219) in the tag-class model (include/serf_sim.h)."""
        self._ck(self.lib.f["set_tags"](self.h, node, tag_class), "sim_set_tags")

    def inject(self, tick, op, node, a=0, b=0):
        self._ck(self.lib.f["inject"](self.h, tick, op, node, a, b), "sim_inject")

    def init_tags(self, classes, first=0):
        """Options::with_tags for the nodes [first, first + len(classes)): start-up tags, no gossip."""
        import numpy as np
        arr = np.ascontiguousarray(classes, dtype=np.uint8)
        self._ck(self.lib.f["init_tags"](self.h, first, len(arr), arr.ctypes.data), "sim_init_tags")

    # ---- the byte boundary of the delegate (delegate.rs:157-163, 317-384) ----
    def inject_record(self, tick, node, key, meta, val):
        """`node` receives the record (key, wire bits of meta, val) at the start of tick `tick` as if it came in a packet."""
        rec = np.zeros(1, REC_DTYPE)
        rec["key"], rec["meta"], rec["val"] = key, meta, val
        self._ck(self.lib.f["inject_record"](self.h, tick, node, rec.ctypes.data), "sim_inject_record")

    def deliver_message(self, node, data: bytes):
        """SerfDelegate::notify_message(buf): one framed serf message in the reference's encoding; returns bytes consumed."""
        used = C.c_size_t()
        self._ck(self.lib.f["deliver_message"](self.h, node, data, len(data), C.byref(used)), "sim_deliver_message")
        return used.value

    def user_event_bytes(self, node, name: bytes, payload: bytes, coalesce=False):
        """Serf::user_event(name, payload, coalesce) (api.rs:241-299) with the bytes themselves."""
        self._ck(self.lib.f["user_event_bytes"](self.h, node, name, len(name), payload, len(payload), int(coalesce)), "sim_user_event_bytes")

    def peek_packet(self, node, k) -> bytes:
        """SerfDelegate::broadcast_messages as bytes: the serf messages of the packet `node` sent in slot k last tick."""
        n = C.c_size_t()
        self._ck(self.lib.f["peek_packet"](self.h, node, k, None, 0, C.byref(n)), "sim_peek_packet")
        buf = np.zeros(max(1, n.value), np.uint8)
        self._ck(self.lib.f["peek_packet"](self.h, node, k, buf.ctypes.data, n.value, C.byref(n)), "sim_peek_packet")
        return buf[:n.value].tobytes()

    def set_stream(self, stream_ptr):
        self._ck(self.lib.f["set_stream"](self.h, C.c_void_p(stream_ptr)), "sim_set_stream")

    # ---- the round's all-to-all issued by the library itself over RCCL (include/serf_sim.h sim_exchange_*) ----
    def exchange_init(self, unique_id: bytes, rank, world):
        self._ck(self.lib.f["exchange_init"](self.h, unique_id, rank, world), "sim_exchange_init")

    def exchange_chunk(self, chunk):
        self._ck(self.lib.f["exchange_chunk"](self.h, chunk), "sim_exchange_chunk")

    def exchange_wait(self):
        self._ck(self.lib.f["exchange_wait"](self.h), "sim_exchange_wait")

    def step(self, n=1):
        self._ck(self.lib.f["step"](self.h, n), "sim_step")

    def sync(self):
        self._ck(self.lib.f["sync"](self.h), "sim_sync")

    @property
    def tick(self):
        t = C.c_uint64()
        self._ck(self.lib.f["tick"](self.h, C.byref(t)), "sim_tick")
        return t.value

    def members(self, observer):
        st = np.zeros(self.n, np.uint8)
        lt = np.zeros(self.n, np.uint64)
        self._ck(self.lib.f["members"](self.h, observer, st.ctypes.data, lt.ctypes.data, self.n), "sim_members")
        return st, lt

    def stats(self, node):
        s = Stats()
        self._ck(self.lib.f["stats_get"](self.h, node, C.byref(s)), "sim_stats_get")
        return s

    def watch(self, observer):
        self._ck(self.lib.f["watch"](self.h, observer), "sim_watch")

    def drain_events(self, cap=65536):
        buf = (Event * cap)()
        n = C.c_uint32()
        self._ck(self.lib.f["drain_events"](self.h, buf, cap, C.byref(n)), "sim_drain_events")
        return [(e.tick, e.observer, e.type, e.key, e.ltime) for e in buf[:n.value]]

    def digest(self):
        d = (C.c_uint64 * 8)()
        self._ck(self.lib.f["state_digest"](self.h, C.byref(d)), "sim_state_digest")
        return tuple(int(x) for x in d)

    def dump(self, which, dtype=None):
        """One state array of the local shard as a structured numpy array (`dtype` overrides the product's record
        layout: an implementation built with other capacity constants has wider rows / buckets)."""
        n = C.c_size_t()
        self._ck(self.lib.f["dump_state"](self.h, which, None, 0, C.byref(n)), "sim_dump_state")
        buf = np.zeros(n.value, np.uint8)
        self._ck(self.lib.f["dump_state"](self.h, which, buf.ctypes.data, n.value, C.byref(n)), "sim_dump_state")
        return buf.view(_ARR_DTYPE[which] if dtype is None else dtype)

    def convergence(self, kind, key, ltime):
        seen, up = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.f["convergence"](self.h, kind, key, ltime, C.byref(seen), C.byref(up)), "sim_convergence")
        return seen.value, up.value

    def convergence_many(self, rumours):
        """([seen_i], up) for a list of up to 64 (kind, key, ltime) in one pass over the nodes."""
        n = len(rumours)
        kinds = (C.c_uint32 * max(1, n))(*[r[0] for r in rumours])
        keys = (C.c_uint32 * max(1, n))(*[r[1] for r in rumours])
        lts = (C.c_uint64 * max(1, n))(*[r[2] for r in rumours])
        seen, up = (C.c_uint64 * max(1, n))(), C.c_uint64()
        self._ck(self.lib.f["convergence_many"](self.h, n, kinds, keys, lts, seen, C.byref(up)), "sim_convergence_many")
        return [int(x) for x in seen[:n]], up.value

    # ---- the extensions: trackers, series, census, roll, ledger, detection log, spread map (include/serf_sim_<group>.h; the oracle has none of them) ----
    def _ext_fn(self, group, name):
        """sim_<group>_<name> of a library that exports the group."""
        if not self.lib.ext[group]:
            raise NotImplementedError(f"{self.lib.path} exports no sim_{group}_* (include/serf_sim_{group}.h)")
        return self.lib.f[f"{group}_{name}"]

    def _sample_count(self, group):
        t, d = C.c_uint32(), C.c_uint32()
        self._ck(self._ext_fn(group, "count")(self.h, C.byref(t), C.byref(d)), f"sim_{group}_count")
        return t.value, d.value

    def _sample_read(self, group, first, n, hdr_dtype, rec_dtype=None, per_sample=0):
        """sim_<group>_read of samples first .. first + n - 1 (n = None: all that were taken from `first` on), each a header and
        per_sample records — the running observer's parameter — split into (headers, records); without rec_dtype a sample is
        one struct (the series) and sim_<group>_read takes no size."""
        fn = self._ext_fn(group, "read")
        if n is None:
            n = max(0, self._sample_count(group)[0] - first)
        stride = (hdr_dtype.itemsize + per_sample * rec_dtype.itemsize if rec_dtype else hdr_dtype.itemsize) // 8
        out = np.zeros(max(1, n) * stride, np.uint64)
        got = C.c_uint32()
        self._ck(fn(self.h, first, n, out.ctypes.data, *([out.size] if rec_dtype else []), C.byref(got)), f"sim_{group}_read")
        words = out[:got.value * stride]
        return sample_split(words, hdr_dtype, rec_dtype, per_sample) if rec_dtype else words.view(hdr_dtype)

    def _sample_stop(self, group):
        self._ck(self._ext_fn(group, "stop")(self.h), f"sim_{group}_stop")

    # ---- device-resident trackers (include/serf_sim_track.h) ----

    def track_add(self, trackers):
        """Registers a list of Tracker; returns their ids (stable until track_remove)."""
        n = len(trackers)
        arr = (Tracker * max(1, n))(*trackers)
        ids = (C.c_uint32 * max(1, n))()
        self._ck(self._ext_fn("track", "add")(self.h, arr, n, ids), "sim_track_add")
        return list(ids[:n])

    def track_remove(self, ids):
        ids = list(ids)
        arr = (C.c_uint32 * max(1, len(ids)))(*ids)
        self._ck(self._ext_fn("track", "remove")(self.h, arr, len(ids)), "sim_track_remove")

    def track_read(self, ids):
        """[TrackResult] of the named trackers; waits for the handle's stream."""
        ids = list(ids)
        arr = (C.c_uint32 * max(1, len(ids)))(*ids)
        out = (TrackResult * max(1, len(ids)))()
        self._ck(self._ext_fn("track", "read")(self.h, arr, len(ids), out), "sim_track_read")
        return list(out[:len(ids)])

    def track_active(self):
        """(registered, of which not retired)."""
        r, a = C.c_uint32(), C.c_uint32()
        self._ck(self._ext_fn("track", "active")(self.h, C.byref(r), C.byref(a)), "sim_track_active")
        return r.value, a.value

    def track_rumour(self, kind, key, ltime, start=0, max_age=0):
        """One RUMOUR tracker (kind = K_JOIN / K_LEAVE / K_EVENT / K_QUERY, as for convergence); returns its id."""
        return self.track_add([rumour_tracker(kind, key, ltime, start, max_age)])[0]

    def track_member(self, subject, status_mask, swim_mask=0, min_inc=0, start=0, max_age=0):
        """One MEMBER tracker: running nodes whose entry of `subject` has a MemberStatus in status_mask (bit i = STATUS_i)
        or, when known, a memberlist state in swim_mask (bit j = SWIM_j), at incarnation >= min_inc; returns its id."""
        return self.track_add([member_tracker(subject, status_mask, swim_mask, min_inc, start, max_age)])[0]

    # ---- device-resident time series (include/serf_sim_series.h) ----
    def series_start(self, first_tick=0, period=1, capacity=1 << 16):
        """Starts sampling: behind every tick t >= first_tick with (t - first_tick) % period == 0, until `capacity` samples
        are held (a first_tick that has passed means "now")."""
        self._ck(self._ext_fn("series", "start")(self.h, first_tick, period, capacity), "sim_series_start")

    def series_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("series")

    def series_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as a numpy array of SERIES_DTYPE;
        waits for the handle's stream."""
        return self._sample_read("series", first, n, SERIES_DTYPE)

    def series_stop(self):
        """Ends the series and frees its buffers (the samples are gone)."""
        self._sample_stop("series")

    # ---- membership census (include/serf_sim_census.h) ----
    def census_start(self, first_tick=0, period=1, capacity=1 << 12, max_subjects=64):
        """Starts a census: behind every tick t >= first_tick with (t - first_tick) % period == 0, until `capacity` samples
        are held (a first_tick that has passed means "now"); a sample keeps the records of the first max_subjects subjects
        in slot order, its header covers all of them."""
        self._ck(self._ext_fn("census", "start")(self.h, first_tick, period, capacity, max_subjects), "sim_census_start")
        self._census_max = max_subjects

    def census_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("census")

    def census_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as (headers, records): numpy
        arrays of CENSUS_HEADER_DTYPE [n] and CENSUS_SUBJECT_DTYPE [n][max_subjects] (a sample's records beyond
        headers["stored"] are zero); waits for the handle's stream."""
        return self._sample_read("census", first, n, CENSUS_HEADER_DTYPE, CENSUS_SUBJECT_DTYPE, getattr(self, "_census_max", 1))

    def census_stop(self):
        """Ends the census and frees its buffers (the samples are gone)."""
        self._sample_stop("census")

    def census_now(self, cap=64):
        """One census of the state the handle is in now, with or without a running one: (header, records[min(subjects,
        cap)]); waits for the handle's stream.  The bulk counterpart of members()."""
        fn = self._ext_fn("census", "now")
        hdr = np.zeros(1, CENSUS_HEADER_DTYPE)
        rec = np.zeros(max(1, cap), CENSUS_SUBJECT_DTYPE)
        got = C.c_uint32()
        self._ck(fn(self.h, hdr.ctypes.data, rec.ctypes.data, cap, C.byref(got)), "sim_census_now")
        return hdr[0], rec[:got.value]

    # ---- observer roll (include/serf_sim_roll.h) ----
    def roll_start(self, first_tick=0, period=1, capacity=1 << 12, top_k=8, rank_by=ROLL_BY_STALE):
        """Starts a roll: behind every tick t >= first_tick with (t - first_tick) % period == 0, until `capacity` samples
        are held (a first_tick that has passed means "now"); a sample keeps the header over all observers and the top_k
        worst of them by `rank_by` (ROLL_BY_STALE / ROLL_BY_ACCUSED / ROLL_BY_MISSED)."""
        self._ck(self._ext_fn("roll", "start")(self.h, first_tick, period, capacity, top_k, rank_by), "sim_roll_start")
        self._roll_top = top_k

    def roll_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("roll")

    def roll_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as (headers, records): numpy
        arrays of ROLL_HEADER_DTYPE [n] and ROLL_NODE_DTYPE [n][top_k] (a sample's records beyond the listed ones are
        zero); waits for the handle's stream."""
        return self._sample_read("roll", first, n, ROLL_HEADER_DTYPE, ROLL_NODE_DTYPE, getattr(self, "_roll_top", 1))

    def roll_stop(self):
        """Ends the roll and frees its buffers (the samples are gone)."""
        self._sample_stop("roll")

    def roll_now(self, top_k=8, rank_by=ROLL_BY_STALE, nodes=False):
        """One roll of the state the handle is in now, with or without a running one: (header, top[top_k]), and with
        nodes=True (header, top[top_k], every node's record [n_nodes]); waits for the handle's stream."""
        fn = self._ext_fn("roll", "now")
        hdr = np.zeros(1, ROLL_HEADER_DTYPE)
        top = np.zeros(max(1, top_k), ROLL_NODE_DTYPE)
        every = np.zeros(self.cfg.n_nodes, ROLL_NODE_DTYPE) if nodes else None
        self._ck(fn(self.h, top_k, rank_by, hdr.ctypes.data, top.ctypes.data, every.ctypes.data if nodes else None), "sim_roll_now")
        return (hdr[0], top[:top_k], every) if nodes else (hdr[0], top[:top_k])

    # ---- rumour ledger (include/serf_sim_ledger.h) ----
    def ledger_start(self, entries=(), first_tick=0, period=1, capacity=1 << 12):
        """Starts a ledger of `entries` ((kind, key, val) triples: a record identity each, 64 at most): behind every tick
        t >= first_tick with (t - first_tick) % period == 0, until `capacity` samples are held (a first_tick that has passed
        means "now"), a header and per entry its reach, holders, queued copies, their transmits, the copies in flight and
        the fresh ones."""
        fn = self._ext_fn("ledger", "start")
        self._ck(fn(self.h, ledger_entries(entries), len(entries), first_tick, period, capacity), "sim_ledger_start")
        self._ledger_n = len(entries)

    def ledger_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("ledger")

    def ledger_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as (headers, records): numpy
        arrays of LEDGER_HEADER_DTYPE [n] and LEDGER_ENTRY_DTYPE [n][entries]; waits for the handle's stream."""
        return self._sample_read("ledger", first, n, LEDGER_HEADER_DTYPE, LEDGER_ENTRY_DTYPE, getattr(self, "_ledger_n", 1))

    def ledger_stop(self):
        """Ends the ledger and frees its buffers (the samples are gone)."""
        self._sample_stop("ledger")

    def ledger_now(self, entries=()):
        """One ledger sample of the state the handle is in now, with or without a running ledger, for entries of its own:
        (header, records[len(entries)]); waits for the handle's stream."""
        fn = self._ext_fn("ledger", "now")
        out = np.zeros(LEDGER_HEADER_WORDS + max(1, len(entries)) * LEDGER_ENTRY_WORDS, np.uint64)
        self._ck(fn(self.h, ledger_entries(entries), len(entries), out.ctypes.data), "sim_ledger_now")
        hdr, rec = ledger_split(out[:LEDGER_HEADER_WORDS + len(entries) * LEDGER_ENTRY_WORDS], len(entries))
        return hdr[0], rec[0]

    # ---- detection log (include/serf_sim_detect.h) ----
    def detect_start(self, first_tick=0, period=1, capacity=1 << 12, log_capacity=1 << 16):
        """Starts a detection log: behind every tick t >= first_tick with (t - first_tick) % period == 0, until `capacity`
        samples are held (a first_tick that has passed means "now"), every view slot's subject is judged — down, or running
        and accused — and the episodes that close are appended to a log of log_capacity records (later ones are counted as
        lost); a sample is a header of cumulative figures."""
        self._ck(self._ext_fn("detect", "start")(self.h, first_tick, period, capacity, log_capacity), "sim_detect_start")

    def detect_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("detect")

    def detect_read(self, first=0, n=None):
        """The headers of samples first .. first + n - 1 (n = None: all that were taken from `first` on) as a numpy array of
        DETECT_HEADER_DTYPE; waits for the handle's stream."""
        fn = self._ext_fn("detect", "read")
        if n is None:
            n = max(0, self._sample_count("detect")[0] - first)
        out = np.zeros(max(1, n), DETECT_HEADER_DTYPE)
        got = C.c_uint32()
        self._ck(fn(self.h, first, n, out.ctypes.data, out.size * DETECT_WORDS, C.byref(got)), "sim_detect_read")
        return out[:got.value]

    def detect_log_count(self):
        """(log records written, lost because the log was full); waits for the handle's stream."""
        w, l = C.c_uint64(), C.c_uint64()
        self._ck(self._ext_fn("detect", "log_count")(self.h, C.byref(w), C.byref(l)), "sim_detect_log_count")
        return w.value, l.value

    def detect_log(self, first=0, n=None):
        """Log records first .. first + n - 1 (n = None: all that were written from `first` on) — the episodes that have
        closed, in (sample, ascending slot) order — as a numpy array of DETECT_EPISODE_DTYPE; waits for the handle's stream."""
        fn = self._ext_fn("detect", "log_read")
        if n is None:
            n = max(0, self.detect_log_count()[0] - first)
        out = np.zeros(max(1, n), DETECT_EPISODE_DTYPE)
        got = C.c_uint32()
        self._ck(fn(self.h, first, n, out.ctypes.data, len(out), C.byref(got)), "sim_detect_log_read")
        return out[:got.value]

    def detect_open(self):
        """The episodes still open (closed = DETECT_NEVER, outcome 0), in ascending slot order, as a numpy array of
        DETECT_EPISODE_DTYPE; waits for the handle's stream."""
        fn = self._ext_fn("detect", "open")
        slots = self.cfg.n_nodes if self.cfg.view_slots == 0 or self.cfg.view_slots >= self.cfg.n_nodes else self.cfg.view_slots
        out = np.zeros(max(1, slots), DETECT_EPISODE_DTYPE)
        got = C.c_uint32()
        self._ck(fn(self.h, out.ctypes.data, len(out), C.byref(got)), "sim_detect_open")
        return out[:got.value]

    def detect_stop(self):
        """Ends the detection log and frees its buffers (samples, log and open episodes are gone)."""
        self._sample_stop("detect")

    # ---- spread map (include/serf_sim_spread.h) ----
    def spread_start(self, entries=(), first_tick=0, period=1, capacity=1 << 12):
        """Starts a spread map of `entries` ((kind, key, ltime) triples of kinds K_JOIN .. K_QUERY, 64 at most): behind every
        tick t >= first_tick with (t - first_tick) % period == 0, until `capacity` samples are held (a first_tick that has
        passed means "now"), every running node that has applied an entry's rumour and has no arrival for it yet gets
        arrival = t + 1; a sample is a header and per entry what it latched and where the entry stands."""
        fn = self._ext_fn("spread", "start")
        self._ck(fn(self.h, spread_entries(entries), len(entries), first_tick, period, capacity), "sim_spread_start")
        self._spread_n = len(entries)

    def spread_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("spread")

    def spread_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as (headers, records): numpy
        arrays of SPREAD_HEADER_DTYPE [n] and SPREAD_ENTRY_DTYPE [n][entries]; waits for the handle's stream."""
        return self._sample_read("spread", first, n, SPREAD_HEADER_DTYPE, SPREAD_ENTRY_DTYPE, getattr(self, "_spread_n", 1))

    def spread_stop(self):
        """Ends the spread map and frees the map and the samples."""
        self._sample_stop("spread")

    def spread_map(self, entry, first_node=0, count=None):
        """arrival[entry][first_node .. first_node + count - 1] (count = None: up to the last node) as a numpy array of
        uint32, 0 = not yet; waits for the handle's stream."""
        if count is None:
            count = max(0, self.cfg.n_nodes - first_node)
        out = np.zeros(max(1, count), np.uint32)
        self._ck(self._ext_fn("spread", "map")(self.h, entry, first_node, count, out.ctypes.data), "sim_spread_map")
        return out[:count]

    def spread_summary(self, bin_width=1):
        """Every entry's summary as a numpy array of SPREAD_SUMMARY_DTYPE [entries]: first and last arrival, the reached,
        the running nodes not reached, the sum and the histogram of arrival - first in bins of bin_width ticks; waits for
        the handle's stream."""
        out = np.zeros(max(1, getattr(self, "_spread_n", 1)), SPREAD_SUMMARY_DTYPE)
        self._ck(self._ext_fn("spread", "summary")(self.h, bin_width, out.ctypes.data), "sim_spread_summary")
        return out[:getattr(self, "_spread_n", 1)]

    def spread_unreached(self, entry, cap=None):
        """(ids, total): the running nodes without an arrival for `entry` in ascending id — the first `cap` of them
        (cap = None: all) — and the number of all of them; waits for the handle's stream."""
        if cap is None:
            cap = self.cfg.n_nodes
        ids = np.zeros(max(1, cap), np.uint32)
        got, total = C.c_uint32(), C.c_uint32()
        self._ck(self._ext_fn("spread", "unreached")(self.h, entry, ids.ctypes.data if cap else None, cap, C.byref(got), C.byref(total)),
                 "sim_spread_unreached")
        return ids[:got.value], total.value

    def spread_late(self, top_k=8, rank_by=SPREAD_BY_MISSED, nodes=False):
        """The top_k worst running nodes by rank_by (SPREAD_BY_MISSED / SPREAD_BY_LATE) as a numpy array of SPREAD_NODE_DTYPE
        [top_k] (records beyond the running nodes are zero), and with nodes=True (top, every node's record [n_nodes]); waits
        for the handle's stream."""
        top = np.zeros(max(1, top_k), SPREAD_NODE_DTYPE)
        every = np.zeros(self.cfg.n_nodes, SPREAD_NODE_DTYPE) if nodes else None
        self._ck(self._ext_fn("spread", "late")(self.h, top_k, rank_by, top.ctypes.data, every.ctypes.data if nodes else None),
                 "sim_spread_late")
        return (top[:top_k], every) if nodes else top[:top_k]

    # ---- traffic meter (include/serf_sim_traffic.h) ----
    def traffic_start(self, first_tick=0, period=1, capacity=1 << 12):
        """Starts the traffic meter: behind every tick t >= first_tick with (t - first_tick) % period == 0, until `capacity`
        samples are held (a first_tick that has passed means "now"), the gossip packets in flight are counted per sender and
        per target into the map (eight uint32 a node, from zero) and summed up in a sample of 64 words."""
        self._ck(self._ext_fn("traffic", "start")(self.h, first_tick, period, capacity), "sim_traffic_start")

    def traffic_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("traffic")

    def traffic_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as a numpy array of TRAFFIC_DTYPE;
        waits for the handle's stream."""
        fn = self._ext_fn("traffic", "read")
        if n is None:
            n = max(0, self._sample_count("traffic")[0] - first)
        out = np.zeros(max(1, n) * TRAFFIC_WORDS, np.uint64)
        got = C.c_uint32()
        self._ck(fn(self.h, first, n, out.ctypes.data, out.size, C.byref(got)), "sim_traffic_read")
        return out[:got.value * TRAFFIC_WORDS].view(TRAFFIC_DTYPE)

    def traffic_stop(self):
        """Ends the meter and frees the map and the samples."""
        self._sample_stop("traffic")

    def traffic_nodes(self, first_node=0, count=None):
        """The map's records of nodes first_node .. first_node + count - 1 (count = None: up to the last node) as a numpy array
        of TRAFFIC_NODE_DTYPE; waits for the handle's stream."""
        if count is None:
            count = max(0, self.cfg.n_nodes - first_node)
        out = np.zeros(max(1, count), TRAFFIC_NODE_DTYPE)
        self._ck(self._ext_fn("traffic", "nodes")(self.h, first_node, count, out.ctypes.data), "sim_traffic_nodes")
        return out[:count]

    def traffic_top(self, top_k=10, column=5):
        """ALL nodes ranked by a column of the map (0 .. 7, TRAFFIC_COLUMN_NAMES; default rx_units) descending, ties by ascending
        id: the first top_k as a numpy array of TRAFFIC_RANK_DTYPE (records beyond n_nodes: id 0xFFFFFFFF and zeros); waits for
        the handle's stream."""
        top = np.zeros(max(1, top_k), TRAFFIC_RANK_DTYPE)
        self._ck(self._ext_fn("traffic", "top")(self.h, top_k, column, top.ctypes.data), "sim_traffic_top")
        return top[:top_k]

    def traffic_summary(self, column=5, bin_width=1):
        """One column of the map over all nodes as a numpy record of TRAFFIC_SUMMARY_DTYPE: sum, max and the smallest id that has
        it, min, the nodes with a non-zero value, the samples accumulated and the histogram in bins of bin_width; waits for the
        handle's stream."""
        out = np.zeros(1, TRAFFIC_SUMMARY_DTYPE)
        self._ck(self._ext_fn("traffic", "summary")(self.h, column, bin_width, out.ctypes.data), "sim_traffic_summary")
        return out[0]

    # ---- rumour tree (include/serf_sim_tree.h) ----
    def tree_start(self, entries=(), first_tick=0, capacity=1 << 12):
        """Starts a rumour tree of `entries` ((kind, key, ltime) triples of kinds K_JOIN .. K_QUERY, 64 at most): behind every
        tick t >= first_tick, until `capacity` samples are held (a first_tick that has passed means "now"), every running node
        that has applied an entry's rumour and has no arrival for it yet gets arrival = t + 1, as its parent the smallest
        sender among the packets with the rumour that the sample before saw addressed to it, and hop = the parent's + 1 (an
        orphan, hop 0, without such a parent)."""
        fn = self._ext_fn("tree", "start")
        self._ck(fn(self.h, spread_entries(entries), len(entries), first_tick, capacity), "sim_tree_start")
        self._tree_n = len(entries)

    def tree_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("tree")

    def tree_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as (headers, records): numpy
        arrays of TREE_HEADER_DTYPE [n] and TREE_ENTRY_DTYPE [n][entries]; waits for the handle's stream."""
        return self._sample_read("tree", first, n, TREE_HEADER_DTYPE, TREE_ENTRY_DTYPE, getattr(self, "_tree_n", 1))

    def tree_stop(self):
        """Ends the tree and frees the planes and the samples."""
        self._sample_stop("tree")

    def tree_links(self, entry, first_node=0, count=None):
        """The links {arrival, parent, hop, children} of nodes first_node .. first_node + count - 1 (count = None: up to the
        last node) in the tree of `entry` as a numpy array of TREE_LINK_DTYPE; waits for the handle's stream."""
        if count is None:
            count = max(0, self.cfg.n_nodes - first_node)
        out = np.zeros(max(1, count), TREE_LINK_DTYPE)
        self._ck(self._ext_fn("tree", "links")(self.h, entry, first_node, count, out.ctypes.data), "sim_tree_links")
        return out[:count]

    def tree_summary(self):
        """Every entry's summary as a numpy array of TREE_SUMMARY_DTYPE [entries]: reached, orphans, depth, the sum of the
        hops, the most children and the smallest id that has them, the histograms of min(hop, 31) and min(children, 31) over
        the reached nodes; waits for the handle's stream."""
        out = np.zeros(max(1, getattr(self, "_tree_n", 1)), TREE_SUMMARY_DTYPE)
        self._ck(self._ext_fn("tree", "summary")(self.h, out.ctypes.data), "sim_tree_summary")
        return out[:getattr(self, "_tree_n", 1)]

    def tree_path(self, entry, node, cap=None):
        """(ids, total): the chain node, parent, grandparent ... up to its orphan — the first `cap` ids (cap = None: all) —
        and its length hop + 1 (0 for a node without an arrival); waits for the handle's stream."""
        if cap is None:
            cap = self.cfg.n_nodes
        ids = np.zeros(max(1, cap), np.uint32)
        got, total = C.c_uint32(), C.c_uint32()
        self._ck(self._ext_fn("tree", "path")(self.h, entry, node, ids.ctypes.data if cap else None, cap, C.byref(got), C.byref(total)),
                 "sim_tree_path")
        return ids[:got.value], total.value

    def tree_top(self, entry, top_k=10):
        """ALL nodes ranked by their children in the tree of `entry` descending, ties by ascending id: the first top_k as a
        numpy array of TREE_RANK_DTYPE (records beyond n_nodes: id 0xFFFFFFFF and zeros); waits for the handle's stream."""
        top = np.zeros(max(1, top_k), TREE_RANK_DTYPE)
        self._ck(self._ext_fn("tree", "top")(self.h, entry, top_k, top.ctypes.data), "sim_tree_top")
        return top[:top_k]

    # ---- query board (include/serf_sim_qboard.h) ----
    @staticmethod
    def _qboard_ids(ids):
        ids = [int(x) for x in ids]
        return (C.c_uint32 * max(1, len(ids)))(*ids), len(ids)

    def qboard_start(self, ids=(), first_tick=0, period=1, capacity=1 << 12):
        """Starts a query board of `ids` (non-zero query ids, 64 at most, running or not yet): behind every tick t >= first_tick
        with (t - first_tick) % period == 0, until `capacity` samples are held (a first_tick that has passed means "now"), every
        query's acks, responses, eligible, answered and silent nodes are counted and its latches moved."""
        arr, n = self._qboard_ids(ids)
        self._ck(self._ext_fn("qboard", "start")(self.h, arr, n, first_tick, period, capacity), "sim_qboard_start")
        self._qboard_n = n

    def qboard_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("qboard")

    def qboard_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as (headers, records): numpy arrays
        of QBOARD_HEADER_DTYPE [n] and QBOARD_ENTRY_DTYPE [n][entries]; waits for the handle's stream."""
        return self._sample_read("qboard", first, n, QBOARD_HEADER_DTYPE, QBOARD_ENTRY_DTYPE, getattr(self, "_qboard_n", 1))

    def qboard_stop(self):
        """Ends the board and frees its records and the samples."""
        self._sample_stop("qboard")

    def qboard_now(self, ids=()):
        """One stateless sample of the state the handle is in now, with or without a running board, for ids of its own:
        (header, records[len(ids)]) with latches and `new` words 0 — n query_status calls with one wait for the stream."""
        arr, n = self._qboard_ids(ids)
        out = np.zeros(QBOARD_HEADER_WORDS + max(1, n) * QBOARD_ENTRY_WORDS, np.uint64)
        self._ck(self._ext_fn("qboard", "now")(self.h, arr, n, out.ctypes.data), "sim_qboard_now")
        hdr, rec = qboard_split(out[:QBOARD_HEADER_WORDS + n * QBOARD_ENTRY_WORDS], n)
        return hdr[0], rec[0]

    def qboard_silent(self, entry, which=0, cap=None):
        """(ids, total): the eligible nodes of `entry` without the ack bit (which 0) or the response bit (which 1) in ascending
        id — the first `cap` of them (cap = None: all) — and the number of all of them; waits for the handle's stream."""
        if cap is None:
            cap = self.cfg.n_nodes
        ids = np.zeros(max(1, cap), np.uint32)
        got, total = C.c_uint32(), C.c_uint32()
        self._ck(self._ext_fn("qboard", "silent")(self.h, entry, which, ids.ctypes.data if cap else None, cap, C.byref(got), C.byref(total)),
                 "sim_qboard_silent")
        return ids[:got.value], total.value

    def qboard_nodes(self, first_node=0, count=None):
        """The records of nodes first_node .. first_node + count - 1 (count = None: up to the last node) over the entries that
        own their table entry now, as a numpy array of QBOARD_NODE_DTYPE; waits for the handle's stream."""
        if count is None:
            count = max(0, self.cfg.n_nodes - first_node)
        out = np.zeros(max(1, count), QBOARD_NODE_DTYPE)
        self._ck(self._ext_fn("qboard", "nodes")(self.h, first_node, count, out.ctypes.data), "sim_qboard_nodes")
        return out[:count]

    def qboard_top(self, top_k=8, rank_by=QBOARD_BY_SILENT_ACK, nodes=False):
        """The top_k worst running nodes by rank_by (QBOARD_BY_SILENT_ACK / QBOARD_BY_SILENT_RESP), ties in ascending id, as a
        numpy array of QBOARD_NODE_DTYPE [top_k] (records beyond the running nodes are zero), and with nodes=True (top, every
        node's record [n_nodes]); waits for the handle's stream."""
        top = np.zeros(max(1, top_k), QBOARD_NODE_DTYPE)
        every = np.zeros(self.cfg.n_nodes, QBOARD_NODE_DTYPE) if nodes else None
        self._ck(self._ext_fn("qboard", "top")(self.h, top_k, rank_by, top.ctypes.data, every.ctypes.data if nodes else None),
                 "sim_qboard_top")
        return (top[:top_k], every) if nodes else top[:top_k]

    # ---- rumour catalogue (include/serf_sim_catalog.h) ----
    def catalog_start(self, kinds_mask=CATALOG_KINDS, max_ids=CATALOG_MAX, first_tick=0, period=1, capacity=1 << 12):
        """Starts a catalogue of the kinds in kinds_mask (bit k: kind k; catalog_mask) with a registry of max_ids records: behind
        every tick t >= first_tick with (t - first_tick) % period == 0, until `capacity` samples are held (a first_tick that has
        passed means "now"), the live record identities are found, counted and entered into the registry."""
        self._ck(self._ext_fn("catalog", "start")(self.h, kinds_mask, max_ids, first_tick, period, capacity), "sim_catalog_start")

    def catalog_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("catalog")

    def catalog_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as a numpy array of
        CATALOG_SAMPLE_DTYPE; waits for the handle's stream."""
        fn = self._ext_fn("catalog", "read")
        if n is None:
            n = max(0, self._sample_count("catalog")[0] - first)
        out = np.zeros(max(1, n), CATALOG_SAMPLE_DTYPE)
        got = C.c_uint32()
        self._ck(fn(self.h, first, n, out.ctypes.data, max(1, n) * CATALOG_SAMPLE_WORDS, C.byref(got)), "sim_catalog_read")
        return out[:got.value]

    def catalog_stop(self):
        """Ends the catalogue and frees the samples and the registry."""
        self._sample_stop("catalog")

    def catalog_list(self, first=0, n=None):
        """Registry records first .. first + n - 1 (n = None: up to the last) as a numpy array of CATALOG_RECORD_DTYPE, in the
        registry's fixed order; waits for the handle's stream."""
        if n is None:
            n = CATALOG_MAX
        out = np.zeros(max(1, n), CATALOG_RECORD_DTYPE)
        got, total = C.c_uint32(), C.c_uint32()
        self._ck(self._ext_fn("catalog", "list")(self.h, first, n, out.ctypes.data, max(1, n) * CATALOG_RECORD_WORDS, C.byref(got),
                                                   C.byref(total)), "sim_catalog_list")
        return out[:got.value]

    def catalog_live(self):
        """The live table of the latest sample taken as a numpy array of CATALOG_LIVE_DTYPE in ascending (id, val) — empty before
        the first sample and after an overflowed one; waits for the handle's stream."""
        out = np.zeros(CATALOG_LIVE, CATALOG_LIVE_DTYPE)
        got = C.c_uint32()
        self._ck(self._ext_fn("catalog", "live")(self.h, out.ctypes.data, CATALOG_LIVE * 8, C.byref(got)), "sim_catalog_live")
        return out[:got.value]

    def catalog_now(self, kinds_mask=CATALOG_KINDS):
        """One scan of the state the handle is in now, with or without a running catalogue, which it does not touch:
        (sample, live table) as CATALOG_SAMPLE_DTYPE and CATALOG_LIVE_DTYPE [live]; it has no registry: the sample's words
        4-8 and 34 are 0."""
        hdr, out = np.zeros(1, CATALOG_SAMPLE_DTYPE), np.zeros(CATALOG_LIVE, CATALOG_LIVE_DTYPE)
        got = C.c_uint32()
        self._ck(self._ext_fn("catalog", "now")(self.h, kinds_mask, hdr.ctypes.data, out.ctypes.data, CATALOG_LIVE * 8, C.byref(got)),
                 "sim_catalog_now")
        return hdr[0], out[:got.value]

    # ---- member gazette (include/serf_sim_gazette.h) ----
    def gazette_start(self, first_tick=0, period=1, capacity=1 << 12, flap_window=60):
        """Starts a gazette: the shadow of every view entry's bits is taken now, and behind every tick t >= first_tick with
        (t - first_tick) % period == 0, until `capacity` samples are held (a first_tick that has passed means "now"), every
        running node's entries are diffed against it: joins, leaves, failures, reaps, flaps (a join out of Failed less than
        flap_window ticks after the failure), suspicions raised and cleared, per node and per subject."""
        self._ck(self._ext_fn("gazette", "start")(self.h, first_tick, period, capacity, flap_window), "sim_gazette_start")

    def gazette_count(self):
        """(samples taken, samples dropped because the buffer was full); waits for nothing."""
        return self._sample_count("gazette")

    def gazette_read(self, first=0, n=None):
        """Samples first .. first + n - 1 (n = None: all that were taken from `first` on) as a numpy array of
        GAZETTE_SAMPLE_DTYPE; waits for the handle's stream."""
        fn = self._ext_fn("gazette", "read")
        if n is None:
            n = max(0, self._sample_count("gazette")[0] - first)
        out = np.zeros(max(1, n), GAZETTE_SAMPLE_DTYPE)
        got = C.c_uint32()
        self._ck(fn(self.h, first, n, out.ctypes.data, max(1, n) * GAZETTE_WORDS, C.byref(got)), "sim_gazette_read")
        return out[:got.value]

    def _gazette_rows(self, which, first, n):
        if n is None:
            n = max(0, self.cfg.n_nodes - first)
        out = np.zeros((max(1, n), GAZETTE_COLS), np.uint32)
        self._ck(self._ext_fn("gazette", which)(self.h, first, n, out.ctypes.data), f"sim_gazette_{which}")
        return out[:n]

    def gazette_nodes(self, first=0, n=None):
        """Rows first .. first + n - 1 (n = None: up to the last node) of the node map as uint32 [n][8] (GAZETTE_COLUMNS): what
        each node's application saw; waits for the handle's stream."""
        return self._gazette_rows("nodes", first, n)

    def gazette_subjects(self, first=0, n=None):
        """The same slice of the subject map: how many observers announced each subject joined, failed, ..."""
        return self._gazette_rows("subjects", first, n)

    def gazette_top(self, which=GAZETTE_MAP_NODES, column=GAZETTE_FAILED, k=10):
        """ALL rows of a map ranked on the device by a column descending, ties by ascending id: the first k as a numpy array
        of GAZETTE_RANK_DTYPE (places beyond n_nodes: id 0xFFFFFFFF and zeros); waits for the handle's stream."""
        top = np.zeros(max(1, k), GAZETTE_RANK_DTYPE)
        self._ck(self._ext_fn("gazette", "top")(self.h, which, column, k, top.ctypes.data), "sim_gazette_top")
        return top[:k]

    def gazette_stop(self):
        """Ends the gazette and frees the samples, the maps and the shadow."""
        self._sample_stop("gazette")

    def snapshot(self):
        """Canonical image of the whole simulated cluster (bytes); restores into any implementation of the ABI."""
        n = C.c_size_t()
        self._ck(self.lib.f["snapshot"](self.h, None, 0, C.byref(n)), "sim_snapshot")
        buf = np.zeros(n.value, np.uint8)
        self._ck(self.lib.f["snapshot"](self.h, buf.ctypes.data, n.value, C.byref(n)), "sim_snapshot")
        return buf

    def restore(self, image):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        self._ck(self.lib.f["restore"](self.h, image.ctypes.data, image.size), "sim_restore")

    def query_status(self, query_id):
        """(acks, responses, still_open) of a running query, as its origin counts them (query.rs:240-303)."""
        a, r, o = C.c_uint64(), C.c_uint64(), C.c_int()
        self._ck(self.lib.f["query_status"](self.h, query_id, C.byref(a), C.byref(r), C.byref(o)), "sim_query_status")
        return a.value, r.value, bool(o.value)

    def query_responders(self, query_id, which):
        """Ids of this shard's nodes whose ack (which = 0) / response (which = 1) reached the origin of the running query —
        what QueryResponse::ack_rx / response_rx deliver (query.rs:201-212), ascending."""
        n = C.c_uint32()
        self._ck(self.lib.f["query_responders"](self.h, query_id, which, None, 0, C.byref(n)), "sim_query_responders")
        out = (C.c_uint32 * max(1, n.value))()
        self._ck(self.lib.f["query_responders"](self.h, query_id, which, out, n.value, C.byref(n)), "sim_query_responders")
        return list(out[:n.value])

    def profile(self, enable=True):
        self._ck(self.lib.f["profile"](self.h, int(enable)), "sim_profile")

    def profile_read(self):
        """(summed tick-kernel milliseconds, launches) since the last read."""
        ms, n = C.c_double(), C.c_uint64()
        self._ck(self.lib.f["profile_read"](self.h, C.byref(ms), C.byref(n)), "sim_profile_read")
        return ms.value, n.value

    def profile_read_stats(self):
        """(sum, min, max) of the timed tick-kernel launches in milliseconds, and their number."""
        ms, n = (C.c_double * 3)(), C.c_uint64()
        self._ck(self.lib.f["profile_read_stats"](self.h, C.byref(ms), C.byref(n)), "sim_profile_read_stats")
        return (ms[0], ms[1], ms[2]), n.value

    def resident_planes(self):
        """{array: (planes with memory, planes)} for view / event ring / query ring, and the bytes of one plane"""
        out = (C.c_uint32 * 6)()
        bpp = C.c_uint64()
        self._ck(self.lib.f["resident_planes"](self.h, out, C.byref(bpp)), "sim_resident_planes")
        return {"view": (out[0], out[1]), "event_ring": (out[2], out[3]), "query_ring": (out[4], out[5]), "bytes_per_plane": bpp.value}

    def cluster_stats(self):
        """Load figures summed over the local shard's nodes (queue depths by class, model-bound drops, ...)."""
        s = ClusterStats()
        self._ck(self.lib.f["cluster_stats_get"](self.h, C.byref(s)), "sim_cluster_stats_get")
        return {"up": s.up, "queued": [int(x) for x in s.queued], "overflow": s.overflow,
                "inbox_records": s.inbox_records, "failed": s.failed, "left": s.left, "max_queue": s.max_queue,
                "ops_dropped": s.ops_dropped, "slots_in_use": s.slots_in_use, "slots_recycled": s.slots_recycled,
                "events_lost": s.events_lost}

    def exchange_bytes(self):
        n = C.c_size_t()
        self._ck(self.lib.f["exchange_bytes"](self.h, C.byref(n)), "sim_exchange_bytes")
        return n.value

    def bind_exchange3(self, send_ptr, send_bytes, recv0_ptr, recv1_ptr, recv_bytes):
        """sim_bind_exchange2 with the sizes of the caller's buffers (SIM_EINVAL when one is too small)"""
        self._ck(self.lib.f["bind_exchange3"](self.h, C.c_void_p(send_ptr), send_bytes, C.c_void_p(recv0_ptr), C.c_void_p(recv1_ptr), recv_bytes), "sim_bind_exchange3")

    def bind_exchange2(self, send_ptr, recv0_ptr, recv1_ptr):
        self._ck(self.lib.f["bind_exchange2"](self.h, C.c_void_p(send_ptr), C.c_void_p(recv0_ptr), C.c_void_p(recv1_ptr)), "sim_bind_exchange2")

    def exchange_chunks(self):
        """(number of sender chunks, bytes of one chunk's region of the exchange buffers)."""
        c, n = C.c_uint32(), C.c_size_t()
        self._ck(self.lib.f["exchange_chunks"](self.h, C.byref(c), C.byref(n)), "sim_exchange_chunks")
        return c.value, n.value

    def exchange_layout(self):
        """(kind, planes, bytes of the send buffer, bytes of the receive buffer) — every kind is an equal-split all-to-all;
        XCHG_ALL_TO_ALL: the slabs of the bijection, written by the tick kernel; XCHG_PACKED: the random fan-out on a shard — the
        slabs are packed from the packets the senders keep, and after a restore the exchange has to be run once more."""
        k, p, a, b = C.c_uint32(), C.c_uint32(), C.c_size_t(), C.c_size_t()
        self._ck(self.lib.f["exchange_layout"](self.h, C.byref(k), C.byref(p), C.byref(a), C.byref(b)), "sim_exchange_layout")
        return k.value, p.value, a.value, b.value

    def pp_due(self):
        return self._ck(self.lib.f["pp_due"](self.h), "sim_pp_due") > 0

    def pp_plan(self, n_shards):
        """(records to send to each peer in round 1, records to receive from each peer, bytes per record)."""
        snd, rcv, rb = (C.c_uint32 * n_shards)(), (C.c_uint32 * n_shards)(), C.c_size_t()
        self._ck(self.lib.f["pp_plan"](self.h, snd, rcv, C.byref(rb)), "sim_pp_plan")
        return list(snd), list(rcv), rb.value

    def pp_export(self, rnd, send_ptr):
        self._ck(self.lib.f["pp_export"](self.h, rnd, C.c_void_p(send_ptr)), "sim_pp_export")

    def pp_merge(self, rnd, recv_ptr):
        self._ck(self.lib.f["pp_merge"](self.h, rnd, C.c_void_p(recv_ptr)), "sim_pp_merge")

    def suspect_requests(self):
        """(prober, target) pairs of the probes that failed on a slot-less target in the tick just ended, sorted by
        prober (sharded hosts: gather, merge, inject OP_SUSPECT on every shard); empties the shard's list."""
        buf = np.zeros((SUSPECT_REQ_MAX, 2), np.uint32)
        n = C.c_uint32()
        self._ck(self.lib.f["suspect_requests"](self.h, buf.ctypes.data, SUSPECT_REQ_MAX, C.byref(n)), "sim_suspect_requests")
        return buf[:n.value].copy()

    def suspect_export(self, out_ptr):
        """Enqueue a copy of the head (SREQ_HEAD_WORDS u32: count + pairs) of the just-ended tick's request list into
        caller memory (device memory for the HIP library)."""
        self._ck(self.lib.f["suspect_export"](self.h, C.c_void_p(out_ptr)), "sim_suspect_export")

    def suspect_import(self, of_tick, heads_ptr, world):
        """The gathered heads of all shards for tick `of_tick` (host memory): merged and scheduled for of_tick + 2."""
        self._ck(self.lib.f["suspect_import"](self.h, of_tick, C.c_void_p(heads_ptr), world), "sim_suspect_import")

    def recycle_due(self):
        return self._ck(self.lib.f["recycle_due"](self.h), "sim_recycle_due") > 0

    def recycle_scan(self):
        """This shard's verdict on the recycling candidates of the next tick: numpy uint32 array [n, 12] (the
        sim_recycle_cand records as words), ready for an all-gather."""
        buf = (RecycleCand * RECYCLE_BATCH)()
        n = C.c_uint32()
        self._ck(self.lib.f["recycle_scan"](self.h, buf, RECYCLE_BATCH, C.byref(n)), "sim_recycle_scan")
        return np.frombuffer(buf, dtype=np.uint32, count=n.value * 12).reshape(n.value, 12).copy()

    def recycle_apply(self, words):
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 12)
        buf = (RecycleCand * max(1, len(words))).from_buffer_copy(words.tobytes() if len(words) else bytes(C.sizeof(RecycleCand)))
        self._ck(self.lib.f["recycle_apply"](self.h, buf, len(words)), "sim_recycle_apply")

    def step_begin(self):
        self._ck(self.lib.f["step_begin"](self.h), "sim_step_begin")

    def step_chunk(self, chunk):
        self._ck(self.lib.f["step_chunk"](self.h, chunk), "sim_step_chunk")

    def step_end(self):
        self._ck(self.lib.f["step_end"](self.h), "sim_step_end")

    def bind_exchange(self, send_ptr, recv_ptr):
        self._ck(self.lib.f["bind_exchange"](self.h, C.c_void_p(send_ptr), C.c_void_p(recv_ptr)), "sim_bind_exchange")
