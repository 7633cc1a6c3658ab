"""Spread map (include/serf_sim_spread.h), the part that needs no GPU: the extension's interface next to the ABI and the six
extensions it must not disturb, the reference model (tests/spread_model.py) against two independent routes on the oracle — the
library's own sim_convergence_many at every tick, and the event log of a run in which every node is watched — the invariants
of the samples, the conditions that make the scenarios non-trivial, and the helper functions on hand-made arrays.

This file owns the scenarios that tests/test_spread_gpu.py runs on the GPU as well.  A scenario is (nodes, configuration, a
script drive(sim, step) that injects every operation up front or between two step(k) calls, ticks); its entries come from a
dry run on the oracle (tests/test_ledger.py: dry_run, deal).

  lives / dies   tests/test_ledger.py's configurations at 512 nodes: kRandomNodes, fan-out 3, six user events from random
                 nodes, one every third tick from tick 2, 60 ticks; `dies` adds loss 0.3 and retransmit_mult 1.  Variants:
                 bijection, vshards_4, lossy (loss 0.03 at least, view slots recycled every 20 ticks)
  series         tests/test_series.py's scenario (six crashes, a revive, a leave, a query, 40 events) at 1 000 nodes with
                 ring_overflow 4 and eight more events sent in ONE tick — one Lamport time, one bucket, eight keys: the
                 bucket continues in an overflow row — 200 ticks, 64 entries of all four kinds

Everything compared is an exact integer."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_abi
from tests import test_ledger as tl
from tests import test_series as ts
from tests.ledger_model import sample as ledger_sample
from tests.spread_model import SpreadModel, node_records, predicate
from tests.test_census import SERIES_SYMBOLS_1
from tests.test_roll import CENSUS_SYMBOLS_1
from tests.test_series import TRACK_SYMBOLS_1
from tests.test_track import ABI_SYMBOLS_15
from tests.test_track_gpu import BIJECTION, KRANDOM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD_HEADER = os.path.join(ROOT, "include", "serf_sim_spread.h")
SPREAD_INC = os.path.join(ROOT, "serf_amd", "csrc", "serf_sim_spread.inc")
LEDGER_SYMBOLS_1 = ("ledger_start", "ledger_count", "ledger_read", "ledger_stop", "ledger_now", "ledger_version")
DETECT_SYMBOLS_1 = ("detect_start", "detect_count", "detect_read", "detect_log_count", "detect_log_read", "detect_open", "detect_stop",
                    "detect_version")
VARIANTS = ("krandomnodes", "bijection", "vshards_4", "lossy")
SPREAD_GRID = 1024                             # serf_sim_spread.inc: #define SPREAD_GRID 1024u; per_pass = gridDim.x * BLOCK


# ---- 1. lives / dies at 512 nodes ----
N, TICKS, EVENTS = 512, 60, 6
BASE = {"lives": dict(tl.LIVES_KW), "dies": dict(tl.DIES_KW)}


def variant_kw(name, variant):
    kw = dict(BASE[name], flags=BIJECTION if variant == "bijection" else KRANDOM)
    if variant == "vshards_4":
        kw["vshards"] = 4
    if variant == "lossy":
        kw.update(loss=max(kw.get("loss", 0.0), 0.03), recycle_interval=20)
    return kw


def events():
    rng = np.random.default_rng(17)
    return [(2 + 3 * i, int(x), 0x51000000 + i) for i, x in enumerate(rng.choice(N, EVENTS, replace=False).tolist())]


def drive(sim, step, ticks=TICKS):
    for t, node, key in events():
        sim.inject(t, _ffi.OP_USER_EVENT, node, key, 64)
    step(ticks)


def model_run(make, script, entries, first=0, period=1, capacity=1 << 12, watch=False):
    """The script on a fresh oracle with a SpreadModel behind the ticks; behind every tick sim_convergence_many of the entries
    and, with watch=True (every node watched), the tick's events.  Returns (oracle, model, [seen per tick], events)."""
    o = make()
    seen, log = [], []
    if watch:
        for x in range(int(o.cfg.n_nodes)):
            o.watch(x)

    def on_tick():
        seen.append(o.convergence_many(entries)[0])
        if watch:
            log.extend(o.drain_events())
    m = SpreadModel(o, on_tick)
    m.start(entries, first, period, capacity)
    script(o, m.step)
    return o, m, seen, log


def event_ltimes(make, script):
    """A dry run on a fresh oracle with every node watched: {event key: the Lamport time its origin gave it}.  (Not the queues:
    with loss 0.3 and retransmit_mult 1 an event whose three packets are all lost is never seen in a queue or in flight behind
    a tick.)"""
    o = make()
    for x in range(int(o.cfg.n_nodes)):
        o.watch(x)
    lts = {}

    def step(k):
        for _ in range(k):
            o.step(1)
            for tick, obs, typ, key, ltime in o.drain_events():
                if typ == _ffi.EV_USER:
                    assert lts.setdefault(key, ltime) == ltime, f"event {key:#x} at two Lamport times"
    script(o, step)
    o.close()
    return lts


@functools.lru_cache(maxsize=None)
def oracle_run(name, variant="krandomnodes"):
    """Once per session; nobody changes what it returns: dict(o, m, entries, samples (headers, records), seen)."""
    make = tl.maker(N, variant_kw(name, variant))
    lts = event_ltimes(make, drive)
    entries = [(_ffi.K_EVENT, key, lts[key]) for _, _, key in events()]
    o, m, seen, _ = model_run(make, drive, entries, capacity=TICKS)
    return dict(o=o, m=m, entries=entries, samples=m.read(), seen=seen)


@functools.lru_cache(maxsize=None)
def watched_run(name):
    """The same run with every node watched (a watched node's row says so: this oracle's digest is not the plain run's):
    (model, the event log)."""
    run = oracle_run(name)
    _, m, _, log = model_run(tl.maker(N, variant_kw(name, "krandomnodes")), drive, run["entries"], capacity=TICKS, watch=True)
    assert words_of(m.read()) == words_of(run["samples"]), "watching changes the spread"
    return m, log


def words_of(samples):
    return [np.ascontiguousarray(a).view(np.uint64).reshape(-1).tolist() for a in samples]


def nonempty_bins(s):
    return (s["bins"] != 0).sum(axis=1)


def check_lives(run):
    """Every entry reaches everybody, over 6 ticks at least (the oracle: 8-9)."""
    tl.inside_bounds(run["o"])
    s = run["m"].summary(1)
    assert (s["unreached_up"] == 0).all() and (s["reached"] == N).all() and (nonempty_bins(s) >= 6).all(), (nonempty_bins(s), s["unreached_up"])
    return s


def check_dies(run):
    """At least four entries leave 32 running nodes or more unreached and spread over 10 ticks or more (the oracle: five
    entries with 79-100 unreached over 12-17 ticks; the sixth never leaves its origin)."""
    tl.inside_bounds(run["o"])
    s = run["m"].summary(1)
    assert ((s["unreached_up"] >= 32) & (nonempty_bins(s) >= 10)).sum() >= 4, (nonempty_bins(s), s["unreached_up"])
    return s


def test_lives_is_nontrivial_on_the_oracle():
    s = check_lives(oracle_run("lives"))
    assert set(nonempty_bins(s).tolist()) <= {8, 9} and s["bins"][0][:8].tolist() == [1, 3, 12, 46, 144, 209, 88, 9]


def test_dies_is_nontrivial_on_the_oracle():
    s = check_dies(oracle_run("dies"))
    spread = s[s["reached"] > 1]
    assert len(spread) == 5 and (spread["unreached_up"] >= 79).all() and (spread["unreached_up"] <= 100).all()
    assert (nonempty_bins(spread) >= 12).all() and (nonempty_bins(spread) <= 17).all()
    assert (s["reached"] == 1).sum() == 1, "one entry never leaves its origin"


# ---- 2. the series scenario: all four kinds, crashes, an overflow row ----
SERIES_N, SERIES_TICKS, SERIES_EVERY = 1000, 200, 6
SERIES_KW = dict(ts.KW, flags=KRANDOM)
SAME_TICK = 8                                   # events of one tick: one Lamport time, one bucket — two keys more than SIM_C


def same_tick_events():
    rng = np.random.default_rng(23)
    s = ts.scenario(SERIES_N)
    nodes = [int(x) for x in rng.permutation(SERIES_N).tolist() if int(x) not in s["crashed"]][:SAME_TICK]
    return [(1, node, 0x30000000 + i) for i, node in enumerate(nodes)]


def series_drive(sim, step, ticks=SERIES_TICKS):
    for t, node, key in same_tick_events():
        sim.inject(t, _ffi.OP_USER_EVENT, node, key, 64)
    ts.drive(sim, ts.scenario(SERIES_N), ticks, step)


def series_entries(found):
    """64 entries of kinds 1-4: the identities found, dealt out as tests/test_ledger.deal does — about 50 — then JOIN and LEAVE
    about the crashed and the live subjects at Lamport time 1 (every baseline holds them: latched at the first sample, for
    subjects with a view slot and without) and at time 2 (held only where a rumour about the subject has arrived)."""
    s = ts.scenario(SERIES_N)
    entries = tl.deal({e for e in found if e[0] <= _ffi.K_QUERY}, _ffi.SPREAD_MAX)
    fill = [(k, x, t) for t in (1, 2) for x in s["crashed"] + s["live"] for k in (_ffi.K_JOIN, _ffi.K_LEAVE)]
    entries += [e for e in fill if e not in entries][:_ffi.SPREAD_MAX - len(entries)]
    return entries


def overflow_entries(o, entries):
    """The EVENT entries some node holds in an OVERFLOW row of the bucket of their Lamport time."""
    n, x, b = int(o.cfg.n_nodes), int(o.cfg.ring_overflow), int(o.cfg.event_ring)
    ring = o.dump(_ffi.ARR_ERING).reshape(-1, n)
    out = []
    for e in entries:
        if e[0] != _ffi.K_EVENT:
            continue
        rows = ring[:x]
        mine = (rows["ltime"].astype(np.int64) & 0xFFFFFFFF) == e[2] % b + 1
        if (mine & (rows["keys"] == e[1]).any(axis=2)).any():
            out.append(e)
    return out


@functools.lru_cache(maxsize=None)
def series_oracle():
    make = tl.maker(SERIES_N, SERIES_KW)
    found, _ = tl.dry_run(make, series_drive, SERIES_EVERY)
    entries = series_entries(found)
    o, m, seen, _ = model_run(make, series_drive, entries, capacity=SERIES_TICKS)
    return dict(o=o, m=m, entries=entries, samples=m.read(), seen=seen)


def check_series(run):
    o, entries, (hdr, rec) = run["o"], run["entries"], run["samples"]
    tl.inside_bounds(o)
    assert len(entries) == _ffi.SPREAD_MAX and {e[0] for e in entries} == {_ffi.K_JOIN, _ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY}
    assert int(o.cfg.ring_overflow) == 4 and overflow_entries(o, entries), "no EVENT entry whose bucket continues in an overflow row"
    assert (rec["reached"] >= rec["reached_up"]).all() and (rec["reached"] > rec["reached_up"]).any(), "no node crashed with an arrival"
    assert hdr["running"].min() < SERIES_N and hdr["started"][-1] >= 60


def test_the_series_scenario_is_nontrivial_on_the_oracle():
    check_series(series_oracle())


# ---- 3. the model against the library's own predicate ----
@pytest.mark.parametrize("name", ("lives", "dies", "series"))
def test_the_models_predicate_summed_is_convergence_many_at_every_tick(name):
    run = series_oracle() if name == "series" else oracle_run(name)
    hdr, rec = run["samples"]
    assert len(run["seen"]) == len(hdr) == (SERIES_TICKS if name == "series" else TICKS)
    assert rec["holds"].tolist() == run["seen"]
    assert rec["holds"].max() > 0
    # the ledger model's reach of the state at the end (its own call of the library) is the last sample's `holds`
    w = ledger_sample(run["o"], run["entries"])
    assert [int(w[8 + 8 * i + 2]) for i in range(len(run["entries"]))] == rec["holds"][-1].tolist()
    # and the predicate alone, without a map behind it, gives the same sum
    holds, up = predicate(run["o"], run["entries"], run["m"].tm)
    assert (holds & up[None, :]).sum(axis=1).tolist() == run["seen"][-1]


# ---- 4. the independent route: the event log ----
@pytest.mark.parametrize("name", ("lives", "dies"))
def test_an_arrival_is_the_tick_behind_the_nodes_user_event(name):
    run = oracle_run(name)
    m, log = watched_run(name)
    first = {}
    for tick, obs, typ, key, ltime in log:
        if typ == _ffi.EV_USER:
            first.setdefault((key, ltime, obs), tick)
    pairs = 0
    for i, (kind, key, ltime) in enumerate(run["entries"]):
        a = m.map(i)
        assert a.tolist() == run["m"].map(i).tolist()
        want = np.zeros(N, np.uint32)
        for x in range(N):
            if (key, ltime, x) in first:
                want[x] = first[(key, ltime, x)] + 1
        assert a.tolist() == want.tolist(), f"entry {i}"
        pairs += int((a != 0).sum())
    assert pairs == int(run["samples"][1]["reached"][-1].sum()) and pairs > N


# ---- 5. invariants ----
@pytest.mark.parametrize("name", ("lives", "dies", "series"))
def test_sample_invariants(name):
    run = series_oracle() if name == "series" else oracle_run(name)
    hdr, rec = run["samples"]
    assert rec["new"].sum(axis=0).tolist() == rec["reached"][-1].tolist()
    assert hdr["new"].tolist() == rec["new"].sum(axis=1).tolist()
    assert (rec["reached"] >= rec["reached_up"]).all() and (rec["holds"] <= hdr["running"][:, None]).all()
    assert (np.diff(rec["reached"].astype(np.int64), axis=0) == rec["new"][1:].astype(np.int64)).all()
    assert hdr["started"].tolist() == (rec["reached"] > 0).sum(axis=1).tolist()
    assert hdr["full"].tolist() == (rec["reached_up"] == hdr["running"][:, None]).sum(axis=1).tolist()
    got = rec["first"] != 0
    assert (got == (rec["reached"] > 0)).all() and (rec["first"] <= rec["last"]).all() and (rec["last"] <= hdr["tick"][:, None]).all()
    m = run["m"]
    s = m.summary(1)
    assert s["reached"].tolist() == rec["reached"][-1].tolist() and s["first"].tolist() == rec["first"][-1].tolist()
    assert (s["bins"].sum(axis=1) == s["reached"]).all() and (s["reached_up"] + s["unreached_up"] == hdr["running"][-1]).all()
    for e in range(len(run["entries"])):
        ids, total = m.unreached(e)
        assert total == len(ids) == s["unreached_up"][e] and (np.diff(ids.astype(np.int64)) > 0).all()
    top, every = m.late(64, _ffi.SPREAD_BY_MISSED, nodes=True)
    assert int(every["got"].sum()) == int(s["reached"].sum()) and (every["got"] + every["missed"] == hdr["started"][-1]).all()
    assert int(every["late_sum"].sum()) == int(s["late_sum"].sum())


# ---- 6. the helper functions on hand-made arrays ----
def test_spread_percentiles_on_hand_made_rows():
    row = np.array([0, 7, 5, 5, 0, 9, 5, 12, 6, 6, 0, 30], np.uint32)           # reached: 5 5 5 6 6 7 9 12 30
    assert _ffi.spread_percentiles(row, [50, 90, 99, 100]) == [6, 30, 30, 30]
    assert _ffi.spread_percentiles(row, [1, 33.3, 33.4, 34, 88.8, 88.9]) == [5, 5, 6, 6, 12, 30]     # (3 of 9 is 33.33 %, 8 of 9 is 88.89 %)
    assert _ffi.spread_percentiles(np.zeros(5, np.uint32), [50, 100]) == [None, None]
    assert _ffi.spread_percentiles(np.array([4], np.uint32), [0.001, 100]) == [4, 4]
    for bad in (0, -1, 100.5):
        with pytest.raises(ValueError):
            _ffi.spread_percentiles(row, [bad])


def test_the_top_k_order_on_hand_made_records_with_ties():
    arrival = np.array([[3, 0, 5, 4, 0, 9, 3, 0],
                        [2, 2, 0, 6, 0, 2, 4, 0],
                        [0, 0, 0, 0, 0, 0, 0, 0]], np.uint32)                     # entry 2 never started
    up = np.array([1, 1, 1, 1, 1, 0, 1, 1], bool)
    first = np.array([3, 2, 0])
    every = node_records(arrival, first, up)
    assert every["got"].tolist() == [2, 1, 1, 2, 0, 2, 2, 0] and every["missed"].tolist() == [0, 1, 1, 0, 2, 0, 0, 2]
    assert every["late_sum"].tolist() == [0, 0, 2, 5, 0, 6, 2, 0] and every["late_max"].tolist() == [0, 0, 2, 4, 0, 6, 2, 0]
    # node 5 does not run: never listed.  missed: 4 and 7 tie (2, late 0): ascending id; then 2 (1, late 2) before 1 (1, late 0)
    assert _ffi.spread_rank(every, _ffi.SPREAD_BY_MISSED) == [4, 7, 2, 1, 3, 6, 0]
    # late: 3 (5); 2 and 6 tie on late 2: missed 1 before missed 0; then late 0: missed 2 (4, 7), missed 1 (1), missed 0 (0)
    assert _ffi.spread_rank(every, _ffi.SPREAD_BY_LATE) == [3, 2, 6, 4, 7, 1, 0]
    assert _ffi.spread_rank(every, _ffi.SPREAD_BY_LATE, 3) == [3, 2, 6] and _ffi.spread_rank(every[:0], _ffi.SPREAD_BY_LATE, 3) == []


# ---- the interface ----
def spread_declared():
    src = re.sub(r"/\*.*?\*/", "", open(SPREAD_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t|const char\s*\*)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_spread_header_declares_what_the_binding_binds():
    assert spread_declared() == sorted("sim_" + s for s in _ffi.SPREAD_SYMBOLS)
    assert len(_ffi.SPREAD_SYMBOLS) == 9


def test_hip_library_exports_the_spread_map():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in spread_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    fn = dll.sim_spread_version
    fn.restype = C.c_uint32
    assert fn() == 1
    assert lib.has_spread and lib.spread_version() == 1


def test_the_abi_and_the_six_older_extensions_are_what_they_were(oracle):
    """The spread map is an extension: serf_sim.h, the six older headers, their symbol lists and the ABI version do not know it;
    the oracle has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == ABI_SYMBOLS_15
    assert tuple(_ffi.TRACK_SYMBOLS) == TRACK_SYMBOLS_1
    assert tuple(_ffi.SERIES_SYMBOLS) == SERIES_SYMBOLS_1
    assert tuple(_ffi.CENSUS_SYMBOLS) == CENSUS_SYMBOLS_1
    assert tuple(_ffi.ROLL_SYMBOLS) == tl.ROLL_SYMBOLS_1
    assert tuple(_ffi.LEDGER_SYMBOLS) == LEDGER_SYMBOLS_1
    assert tuple(_ffi.DETECT_SYMBOLS) == DETECT_SYMBOLS_1
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in ABI_SYMBOLS_15)
    assert tl.ledger_declared() == sorted("sim_" + s for s in LEDGER_SYMBOLS_1)
    older = set(_ffi.ABI_SYMBOLS) | set(_ffi.TRACK_SYMBOLS) | set(_ffi.SERIES_SYMBOLS) | set(_ffi.CENSUS_SYMBOLS) | set(_ffi.ROLL_SYMBOLS)
    older |= set(_ffi.LEDGER_SYMBOLS) | set(_ffi.DETECT_SYMBOLS)
    assert not set(_ffi.SPREAD_SYMBOLS) & older
    lib = serf_amd.load()
    assert lib.abi_version() == 15 and oracle.abi_version() == 15
    assert lib.track_version() == 1 and lib.series_version() == 1 and lib.census_version() == 1 and lib.roll_version() == 1
    assert lib.ledger_version() == 1 and lib.detect_version() == 1
    dll = C.CDLL(lib.path)
    for s in older:
        assert hasattr(dll, "sim_" + s), s
    assert not oracle.has_spread and oracle.spread_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.SPREAD_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)
    o = _ffi.Sim(oracle, _ffi.make_config(64))
    e = [(_ffi.K_JOIN, 1, 1)]
    for call in (lambda: o.spread_start(e), o.spread_count, o.spread_read, o.spread_stop, lambda: o.spread_map(0), o.spread_summary,
                 lambda: o.spread_unreached(0), o.spread_late):
        with pytest.raises(NotImplementedError):
            call()


def test_spread_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "serf_sim_spread.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %u %u %u %u %u %u %u %u %u %u %u %u\\n",sizeof(sim_spread_entry),'
                    "offsetof(sim_spread_entry,key),offsetof(sim_spread_entry,ltime),sizeof(sim_spread_node),SIM_SPREAD_MAX,"
                    "SIM_SPREAD_MAX_SAMPLES,SIM_SPREAD_VERSION,SIM_SPREAD_HEADER_WORDS,SIM_SPREAD_ENTRY_WORDS,SIM_SPREAD_BINS,"
                    "SIM_SPREAD_SUMMARY_WORDS,SIM_SPREAD_TOP_MAX,SIM_SPREAD_NODE_WORDS,SIM_SPREAD_BY_MISSED,SIM_SPREAD_BY_LATE,SIM_CONV_MAX);"
                    "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_ffi.SpreadEntry), _ffi.SpreadEntry.key.offset, _ffi.SpreadEntry.ltime.offset, _ffi.SPREAD_NODE_DTYPE.itemsize,
                   _ffi.SPREAD_MAX, _ffi.SPREAD_MAX_SAMPLES, 1, _ffi.SPREAD_HEADER_WORDS, _ffi.SPREAD_ENTRY_WORDS, _ffi.SPREAD_BINS,
                   _ffi.SPREAD_SUMMARY_WORDS, _ffi.SPREAD_TOP_MAX, _ffi.SPREAD_NODE_WORDS, _ffi.SPREAD_BY_MISSED, _ffi.SPREAD_BY_LATE, 64]
    assert got[:5] == [16, 4, 8, 64, 64] and C.sizeof(_ffi.SpreadEntry) == C.sizeof(_ffi.LedgerEntry)
    off = {n: _ffi.SPREAD_HEADER_DTYPE.fields[n][1] // 8 for n in _ffi.SPREAD_HEADER_DTYPE.names}
    assert off == dict(tick=0, running=1, n=2, new=3, started=4, full=5, reserved=6)
    off = {n: _ffi.SPREAD_ENTRY_DTYPE.fields[n][1] // 8 for n in _ffi.SPREAD_ENTRY_DTYPE.names}
    assert off == dict(id=0, val=1, new=2, reached=3, reached_up=4, holds=5, first=6, last=7)
    off = {n: _ffi.SPREAD_SUMMARY_DTYPE.fields[n][1] // 8 for n in _ffi.SPREAD_SUMMARY_DTYPE.names}
    assert off == dict(id=0, val=1, first=2, last=3, reached=4, reached_up=5, unreached_up=6, late_sum=7, bins=8)
    off = {n: _ffi.SPREAD_NODE_DTYPE.fields[n][1] for n in _ffi.SPREAD_NODE_DTYPE.names}
    assert off == dict(id=0, running=4, got=8, missed=16, late_sum=24, late_max=32, reserved=40)
    for n in (1, 5, 64):
        hdr, rec = _ffi.spread_split(np.arange(3 * (8 + 8 * n), dtype=np.uint64), n)
        assert hdr.shape == (3,) and rec.shape == (3, n) and hdr["tick"].tolist() == [0, 8 + 8 * n, 2 * (8 + 8 * n)]
        assert rec["last"][1, n - 1] == 2 * (8 + 8 * n) - 1


def test_the_cap_is_the_sources():
    """SPREAD_GRID above mirrors these lines; a change there has to move the second-pass size of tests/test_spread_gpu.py."""
    src = open(SPREAD_INC).read()
    assert re.search(r"^#define SPREAD_GRID %du\b" % SPREAD_GRID, src, re.M)
    assert src.count("const size_t per_pass = (size_t)gridDim.x * BLOCK;") == 3        # the latch kernel and the summary's two passes
    assert "p.G = spread_grid(h);" in src and "std::min<size_t>(((size_t)h->d.Nl + BLOCK - 1) / BLOCK, SPREAD_GRID)" in src
    assert re.search(r"^#define BLOCK 256$", open(os.path.join(ROOT, "serf_amd", "csrc", "serf_sim.hip")).read(), re.M)
