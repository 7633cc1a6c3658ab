"""Rumour ledger (include/serf_sim_ledger.h), the part that needs no GPU: the extension's interface next to the ABI and the four
extensions it must not disturb, the reference model (tests/ledger_model.py) against independent routes on the oracle (the series
model, the tracker model's view count, the queue depths), and ledger_summary on hand-made arrays.

This file owns the scenarios that tests/test_ledger_gpu.py runs on the GPU as well.  A scenario is (nodes, configuration, a script
drive(sim, step) that injects every operation up front or between two step(k) calls, ticks); its entries come from a dry run on
the oracle: the identities of the queued records of running nodes, collected behind the ticks t with t % every == every - 1,
sorted ascending and dealt out round-robin over the kinds in ascending kind until 64 are taken (deal).

  dies / lives   4 096 nodes, kRandomNodes, fan-out 3, six user events from random nodes, one every third tick, 60 ticks.  With
                 loss 0.3 and retransmit_mult 1 every event stops being carried before it has reached everybody; without loss and
                 with the default multiplier every event reaches everybody and the cluster sends exactly 16 copies per node
  census         the four variants of tests/test_census.py (census_drive, census_kw) at 4 096 nodes, 200 ticks
  deep           the third configuration of tests/test_bounds.py: 512 nodes, pkt_records 8 (two pages), queues up to 50 deep,
                 all seven kinds
  pages          `lives` with pkt_records 16 and 12 events in one tick from one node: packets of four pages
  twice          one node sends the same event key twice: two entries that differ in val only

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
from tests import _scenario as sc
from tests import test_abi
from tests._oracle import load_oracle
from tests.ledger_model import LedgerModel, identities, queued_records, sample, wire_records
from tests.series_model import sample as series_sample
from tests.test_census import SERIES_SYMBOLS_1, census_drive, census_kw
from tests.test_roll import CENSUS_SYMBOLS_1
from tests.test_series import TRACK_SYMBOLS_1, scenario
from tests.test_track import ABI_SYMBOLS_15
from tests.test_track_gpu import KRANDOM
from tests.track_model import TrackModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER_HEADER = os.path.join(ROOT, "include", "serf_sim_ledger.h")
LEDGER_INC = os.path.join(ROOT, "serf_amd", "csrc", "serf_sim_ledger.inc")
ROLL_SYMBOLS_1 = ("roll_start", "roll_count", "roll_read", "roll_stop", "roll_now", "roll_version")
N = 4096
VARIANTS = ("krandomnodes", "bijection", "vshards_4", "lossy")
RUMOURS = (_ffi.K_JOIN, _ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY)


# ---- entries by dry run ----
def deal(found, limit=_ffi.LEDGER_MAX):
    """Identities sorted ascending, dealt out round-robin over the kinds in ascending kind until `limit` are taken."""
    by_kind = {k: sorted(e for e in found if e[0] == k) for k in range(1, 8)}
    out, r = [], 0
    while len(out) < limit and any(len(v) > r for v in by_kind.values()):
        for k in range(1, 8):
            if len(by_kind[k]) > r and len(out) < limit:
                out.append(by_kind[k][r])
        r += 1
    return out


def dry_run(make, drive, every=1, wire=False):
    """The script on a fresh oracle, one tick at a time.  Returns (the identities found behind the ticks t with t % every ==
    every - 1, the deepest queue of a running node at any tick).  wire=True: the identities of the records in flight as well
    (below ten nodes a record's four transmits are one tick's packets: it is never in a queue behind a tick)."""
    o = make()
    found, deepest = set(), [0]

    def step(k):
        for _ in range(k):
            o.step(1)
            if (o.tick - 1) % every == every - 1:
                found.update(identities(o))
                if wire:
                    wk, wkey, wval, _ = wire_records(o)
                    found.update(zip(wk.tolist(), wkey.tolist(), wval.tolist()))
                node = queued_records(o)[0]
                if len(node):
                    deepest[0] = max(deepest[0], int(np.bincount(node).max()))
    drive(o, step)
    o.close()
    return found, deepest[0]


def model_run(make, drive, entries, first=0, period=1, capacity=1 << 12, probe=None):
    """The script on a fresh oracle with a LedgerModel behind the ticks.  probe(o), when given, runs behind every tick; its
    results come back as a list.  Returns (oracle, model, probed)."""
    o = make()
    probed = []
    m = LedgerModel(o, (lambda: probed.append(probe(o))) if probe else None)
    m.start(entries, first, period, capacity)
    drive(o, m.step)
    return o, m, probed


def inside_bounds(o):
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0            # the run stays inside the model's bounds
    return cs


def maker(n, kw):
    return lambda: _ffi.Sim(load_oracle(), _ffi.make_config(n, **kw))


# ---- 1. a rumour that dies, and the same script where it lives ----
DIES_TICKS, DIES_EVENTS = 60, 6
DIES_BASE = dict(fanout=3, view_slots=64, event_ring=64, query_ring=64, flags=KRANDOM)
DIES_KW = dict(DIES_BASE, loss=0.3, retransmit_mult=1)
LIVES_KW = dict(DIES_BASE)


def dies_events():
    rng = np.random.default_rng(17)
    return [(2 + 3 * i, int(x), 0x51000000 + i) for i, x in enumerate(rng.choice(N, DIES_EVENTS, replace=False).tolist())]


def dies_drive(sim, step, ticks=DIES_TICKS):
    for t, node, key in dies_events():
        sim.inject(t, _ffi.OP_USER_EVENT, node, key, 64)
    step(ticks)


def event_entries(found, keys):
    """The EVENT identities of the listed keys, in the keys' order (a key once: its only Lamport time)."""
    out = []
    for key in keys:
        got = sorted(e for e in found if e[0] == _ffi.K_EVENT and e[1] == key)
        assert got, f"event {key:#x} was never queued"
        out += got
    return out


@functools.lru_cache(maxsize=None)
def dies_oracle(lossy):
    """Once per session; nobody changes what it returns: (oracle, entries, (headers, records))."""
    make = maker(N, DIES_KW if lossy else LIVES_KW)
    found, _ = dry_run(make, dies_drive)
    entries = event_entries(found, [key for _, _, key in dies_events()])
    assert len(entries) == DIES_EVENTS
    o, m, _ = model_run(make, dies_drive, entries, capacity=DIES_TICKS)
    return o, entries, m.read()


def check_dies(run):
    o, entries, (hdr, rec) = run
    inside_bounds(o)
    assert hdr["tick"].tolist() == list(range(1, DIES_TICKS + 1)) and rec.shape == (DIES_TICKS, DIES_EVENTS)
    summ = _ffi.ledger_summary(hdr, rec)
    for i, ((t0, node, key), s) in enumerate(zip(dies_events(), summ)):
        r = rec[:, i]
        carried = r["queued"].astype(np.int64) + r["in_flight"].astype(np.int64)
        assert (carried[-5:] == 0).all() and (r["reach"][-5:] < hdr["running"][-5:]).all(), f"event {i} was to die before it reached everybody"
        assert r["reach"][-1] > N // 2 and carried.max() > 0
        assert s["died_at"] is not None and s["reach_at_death"] <= s["reach"] < s["running"] == N
        assert s["first_tick"] == t0 + 1 and 8 <= s["died_at"] - t0 <= 40
        assert (r["fresh"] <= r["queued"]).all() and (r["holders"] <= r["queued"]).all()
    return summ


def check_lives(run):
    o, entries, (hdr, rec) = run
    inside_bounds(o)
    assert rec.shape == (DIES_TICKS, DIES_EVENTS)
    for i in range(DIES_EVENTS):
        r = rec[:, i]
        assert r["reach"][-1] == hdr["running"][-1] == N
        assert int(r["in_flight"].astype(np.int64).sum()) == 16 * N, "16 copies per node (retransmit_mult 4 x 4 digits)"
        assert r["queued"][-1] == 0 and r["in_flight"][-1] == 0
    summ = _ffi.ledger_summary(hdr, rec)
    assert all(s["copies_per_node"] == 16.0 and s["died_at"] is not None and s["reach_at_death"] == N for s in summ)


def test_a_rumour_that_dies_on_the_oracle():
    check_dies(dies_oracle(True))


def test_the_same_script_without_loss_on_the_oracle():
    check_lives(dies_oracle(False))


# ---- 2. the fan-out models ----
CENSUS_TICKS, EVERY = 200, 6


def census_ledger_drive(sim, step):
    census_drive(sim, scenario(N), CENSUS_TICKS, step)


@functools.lru_cache(maxsize=None)
def census_oracle(variant):
    make = maker(N, census_kw(variant))
    found, _ = dry_run(make, census_ledger_drive, EVERY)
    entries = deal(found)
    o, m, _ = model_run(make, census_ledger_drive, entries, capacity=CENSUS_TICKS)
    return o, entries, m.read()


def check_census(variant, run):
    o, entries, (hdr, rec) = run
    inside_bounds(o)
    assert 40 <= len(entries) <= _ffi.LEDGER_MAX and hdr["tick"].tolist() == list(range(1, CENSUS_TICKS + 1))
    kinds = {e[0] for e in entries}
    assert {_ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY, _ffi.K_SUSPECT, _ffi.K_DEAD} <= kinds
    assert (rec["queued"].max(axis=0) > 0).all(), "every entry was found in a queue: it is queued at some tick"
    assert (rec["in_flight"].max(axis=0) > 0).sum() >= len(entries) // 2 and hdr["packets"].max() > 0
    reach = rec["reach"]
    for i, e in enumerate(entries):
        assert (reach[:, i] == 0).all() if e[0] not in RUMOURS else reach[:, i].max() > 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_census_scenarios_on_the_oracle(variant):
    check_census(variant, census_oracle(variant))


# ---- 3. deep queues, two pages, all seven kinds ----
DEEP_N, DEEP_TICKS = 512, 72
DEEP_KW = dict(fanout=4, event_ring=32, query_ring=16, leave_delay=6, probe_interval=4, loss=0.01, pkt_records=8, reap_interval=7,
               reconnect_timeout=60, tombstone_timeout=80, intent_timeout=30, queue_check_interval=9, push_pull_interval=6,
               flags=_ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT, view_slots=96, ring_overflow=8)
DEEP_FOUND = {1: 2, 2: 18, 3: 39, 4: 15, 5: 9, 6: 15, 7: 13}       # identities by kind, behind every sixth tick
DEEP_DEALT = {1: 2, 2: 11, 3: 11, 4: 11, 5: 9, 6: 10, 7: 10}


def deep_drive(sim, step):
    sc.apply_schedule(sim, sc.schedule(DEEP_N, 40, rate=2.0, seed=524, max_member_subjects=40))
    step(DEEP_TICKS)


def deep_probe(o):
    """Behind every tick: (series words 3 .. 5 as the ledger's header names them, the deepest queue, the total depth)."""
    w = series_sample(o)
    node = queued_records(o)[0]
    depth = np.bincount(node, minlength=1)
    return int(w[6:10].sum()), int(w[41:48].sum()), int(w[40]), int(depth.max()), int(depth.sum())


def by_kind(entries):
    return {k: sum(1 for e in entries if e[0] == k) for k in range(1, 8)}


@functools.lru_cache(maxsize=None)
def deep_oracle():
    make = maker(DEEP_N, DEEP_KW)
    found, deepest = dry_run(make, deep_drive, EVERY)
    entries = deal(found)
    o, m, probed = model_run(make, deep_drive, entries, capacity=DEEP_TICKS, probe=deep_probe)
    return o, entries, m.read(), probed, by_kind(found), found


def check_deep(run):
    o, entries, (hdr, rec), probed, found_by_kind, _ = run
    inside_bounds(o)
    assert found_by_kind == DEEP_FOUND and by_kind(entries) == DEEP_DEALT
    assert max(p[3] for p in probed) > _ffi.Q_HOT, "no deep queue"
    for k in range(1, 8):
        cols = [i for i, e in enumerate(entries) if e[0] == k]
        assert rec["queued"][:, cols].max() > 0 and rec["in_flight"][:, cols].max() > 0, f"kind {k} never queued or never in flight"
    assert (rec["queued"].max(axis=0) > 0).all(), "an entry that is never carried"
    assert (rec["queued"] > rec["holders"]).any(), "no node ever holds two records of one identity"
    return hdr, rec


def test_deep_queues_on_the_oracle_and_three_independent_routes():
    run = deep_oracle()
    hdr, rec = check_deep(run)
    o, entries, _, probed, _, found = run
    # words 3 .. 5 of the header: the series model's words
    assert hdr["queued"].tolist() == [p[0] for p in probed] and hdr["in_flight"].tolist() == [p[1] for p in probed]
    assert hdr["packets"].tolist() == [p[2] for p in probed]
    assert (hdr["transmits"] > 0).any() and (rec["transmits"].sum(axis=1) <= hdr["transmits"]).all()
    # some node deeper than SIM_Q_HOT holds a match of an entry (the state at the end of a fresh run up to the deepest tick)
    deepest_tick = int(np.argmax([p[3] for p in probed]))
    m = maker(DEEP_N, DEEP_KW)()
    deep_drive(m, lambda k: m.step(deepest_tick + 1))
    node, kind, key, val, _, _ = queued_records(m)
    depth = np.bincount(node, minlength=DEEP_N)
    listed = set(entries)
    assert any(depth[x] > _ffi.Q_HOT and (k, y, v) in listed for x, k, y, v in zip(node.tolist(), kind.tolist(), key.tolist(), val.tolist()))
    # holders summed over ALL identities that occur now: between the largest depth and the total depth
    now = sorted(identities(m))
    holders = 0
    for j in range(0, len(now), _ffi.LEDGER_MAX):
        _, r = _ffi.ledger_split(sample(m, now[j:j + _ffi.LEDGER_MAX]), len(now[j:j + _ffi.LEDGER_MAX]))
        holders += int(r["holders"].sum())
        assert (r["queued"] > 0).all()
    assert depth.max() <= holders <= depth.sum() and depth.max() > _ffi.Q_HOT
    # reach of the JOIN / LEAVE entries: the tracker model's count over the view dump (no convergence call in that route)
    tm = TrackModel(o)
    slot, view, up = tm._dumps()
    checked = 0
    for i, e in enumerate(entries):
        if e[0] in (_ffi.K_JOIN, _ffi.K_LEAVE):
            assert int(rec["reach"][-1, i]) == tm.count_view(_ffi.rumour_tracker(*e), slot, view, up), e
            checked += 1
    assert checked >= 10 and rec["reach"][-1].max() > 0
    m.close()


# ---- 4. four pages ----
PAGES_TICKS, PAGES_NODE, PAGES_EVENTS = 40, 1234, 12
PAGES_KW = dict(LIVES_KW, pkt_records=16)


def pages_keys():
    return [0x52000000 + i for i in range(PAGES_EVENTS)]


def pages_drive(sim, step):
    for key in pages_keys():
        sim.inject(2, _ffi.OP_USER_EVENT, PAGES_NODE, key, 64)
    step(PAGES_TICKS)


def pages_probe(o):
    """Records in the fullest packet in flight: beyond 12 means a fourth page is in use."""
    n = int(o.cfg.n_nodes)
    hm = o.dump(_ffi.ARR_INBOX).reshape(-1, n)["hi_meta"].astype(np.int64)
    f = int(o.cfg.fanout)
    return int((((hm >> 4) & 0xF) != 0).reshape(f, -1, n, 4).sum(axis=(1, 3)).max())


@functools.lru_cache(maxsize=None)
def pages_oracle():
    make = maker(N, PAGES_KW)
    found, _ = dry_run(make, pages_drive)
    entries = event_entries(found, pages_keys())
    o, m, probed = model_run(make, pages_drive, entries, capacity=PAGES_TICKS, probe=pages_probe)
    return o, entries, m.read(), probed


def check_pages(run):
    o, entries, (hdr, rec), probed = run
    inside_bounds(o)
    assert len(entries) == PAGES_EVENTS and max(probed) == PAGES_EVENTS, "a packet was to carry all twelve events: three full pages"
    assert (rec["reach"][-1] == N).all() and (rec["in_flight"].astype(np.int64).sum(axis=0) == 16 * N).all()
    assert (hdr["in_flight"] > 8 * hdr["packets"]).any(), "packets of more than two pages on average"


def test_four_pages_on_the_oracle():
    check_pages(pages_oracle())


# ---- 5. one pair, several values ----
TWICE_N, TWICE_TICKS, TWICE_KEY, TWICE_NODE = 1024, 40, 0x53000001, 77
TWICE_KW = dict(LIVES_KW, probe_interval=5)
TWICE_SUSPECT = (_ffi.K_SUSPECT, 9)            # a SUSPECT of subject 9 at incarnations 0 and 1, put into node 5's and node 6's hands
WIRE_META = lambda kind: ((63 - 2) << 18) | (kind << 4)       # len64 2, no flags


def twice_drive(sim, step):
    sim.inject(2, _ffi.OP_USER_EVENT, TWICE_NODE, TWICE_KEY, 64)
    sim.inject(9, _ffi.OP_USER_EVENT, TWICE_NODE, TWICE_KEY, 64)
    for inc, node in ((0, 5), (1, 6)):
        sim.inject_record(4, node, TWICE_SUSPECT[1], WIRE_META(_ffi.K_SUSPECT), inc | (3 << 32))
    step(TWICE_TICKS)


@functools.lru_cache(maxsize=None)
def twice_oracle():
    make = maker(TWICE_N, TWICE_KW)
    found, _ = dry_run(make, twice_drive)
    ev = sorted(e for e in found if e[0] == _ffi.K_EVENT and e[1] == TWICE_KEY)
    su = sorted(e for e in found if e[:2] == TWICE_SUSPECT)
    o, m, _ = model_run(make, twice_drive, ev + su, capacity=TWICE_TICKS)
    return o, ev + su, m.read(), (ev, su)


def check_twice(run):
    o, entries, (hdr, rec), (ev, su) = run
    assert len(ev) == 2 and ev[0][2] < ev[1][2], "one key at two Lamport times"
    i0, i1 = 0, 1
    assert rec["queued"][:, i0].max() > 0 and rec["queued"][:, i1].max() > 0
    both = (rec["queued"][:, i0] > 0) & (rec["queued"][:, i1] > 0)
    assert both.any(), "the two were to travel at the same time"
    assert rec["reach"][-1, i0] == rec["reach"][-1, i1] == hdr["running"][-1]
    assert (rec["reach"][:, i1] <= rec["reach"][:, i0]).all() and (rec["reach"][:, i1] < rec["reach"][:, i0]).any()
    if len(su) == 2:                     # the same subject suspected at two incarnations: entries that differ in val only
        j0, j1 = 2, 3
        assert rec["queued"][:, j0].max() > 0 and rec["queued"][:, j1].max() > 0
    return len(su)


def test_one_pair_two_values_on_the_oracle():
    assert check_twice(twice_oracle()) == 2, "both SUSPECT records were to be queued"


# ---- 6. a crowded index ----
def ledger_tab():
    """The size of the LDS index, from the source."""
    m = re.search(r"^#define LEDGER_TAB (\d+)u\b", open(LEDGER_INC).read(), re.M)
    assert m, "serf_sim_ledger.inc no longer defines LEDGER_TAB"
    return int(m.group(1))


def ledger_bucket(kind, key):
    """serf_sim_ledger.inc: ledger_bucket."""
    return ((key * 0x9E3779B1 + kind * 0x85EBCA6B) & 0xFFFFFFFF) >> 25


def crowded_entries(real):
    """64 entries: `real` (the six events of `dies`), in front of each of the first two seven made-up events of its bucket —
    so that the real entry stands at the END of a chain of eight — the rest made-up LEAVEs about low subjects."""
    out, used = [], set(real)
    for e in real[:2]:
        key, b = 1, ledger_bucket(e[0], e[1])
        fill = []
        while len(fill) < 7:
            key += 1
            if ledger_bucket(_ffi.K_EVENT, key) == b and (_ffi.K_EVENT, key, e[2]) not in used:
                fill.append((_ffi.K_EVENT, key, e[2]))
        out += fill + [e]
        used.update(fill)
    out += list(real[2:])
    s = 0
    while len(out) < _ffi.LEDGER_MAX:
        out.append((_ffi.K_LEAVE, s, 7))
        s += 1
    return out


def longest_chain(entries):
    return max(np.bincount([ledger_bucket(e[0], e[1]) for e in entries]))


def test_the_index_is_the_sources():
    """ledger_bucket above mirrors these lines; a change there has to move crowded_entries."""
    src = open(LEDGER_INC).read()
    assert ledger_tab() == 128
    assert "static inline u32 ledger_bucket(u32 kind, u32 key) { return (key * 0x9E3779B1u + kind * 0x85EBCA6Bu) >> 25; }" in src
    assert re.search(r"^#define LEDGER_GRID 1024u\b", src, re.M) and "const size_t per_pass = (size_t)gridDim.x * BLOCK;" in src
    assert all(0 <= ledger_bucket(k, key) < ledger_tab() for k in range(1, 8) for key in (0, 1, 77, 0xFFFFFFFF))


@functools.lru_cache(maxsize=None)
def crowded_oracle():
    _, real, _ = dies_oracle(True)
    entries = crowded_entries(list(real))
    o, m, _ = model_run(maker(N, DIES_KW), lambda sim, step: dies_drive(sim, step, 30), entries, period=3, capacity=10)
    return o, entries, m.read()


def check_crowded(run):
    o, entries, (hdr, rec) = run
    assert len(entries) == len(set(entries)) == _ffi.LEDGER_MAX and longest_chain(entries) >= 8
    real = [i for i, e in enumerate(entries) if e[0] == _ffi.K_EVENT and e[1] >> 24 == 0x51]
    assert len(real) == DIES_EVENTS and real[:2] == [7, 15]
    assert (rec["queued"][:, real].max(axis=0) > 0).all() and (rec["in_flight"][:, real].max(axis=0) > 0).all()
    others = [i for i in range(len(entries)) if i not in real]
    for f in ("holders", "queued", "transmits", "in_flight", "fresh"):
        assert not rec[f][:, others].any()


def test_a_crowded_index_on_the_oracle():
    check_crowded(crowded_oracle())


# ---- the interface ----
def ledger_declared():
    src = re.sub(r"/\*.*?\*/", "", open(LEDGER_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t|const char\s*\*)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_ledger_header_declares_what_the_binding_binds():
    assert ledger_declared() == sorted("sim_" + s for s in _ffi.LEDGER_SYMBOLS)
    assert len(_ffi.LEDGER_SYMBOLS) == 6


def test_hip_library_exports_the_ledger():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in ledger_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    fn = dll.sim_ledger_version
    fn.restype = C.c_uint32
    assert fn() == 1
    assert lib.has_ledger and lib.ledger_version() == 1


def test_the_abi_and_the_four_older_extensions_are_what_they_were(oracle):
    """The ledger is an extension: serf_sim.h, the four older headers, their symbol lists and the ABI version do not know it;
    the oracle has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == ABI_SYMBOLS_15
    assert tuple(_ffi.TRACK_SYMBOLS) == TRACK_SYMBOLS_1
    assert tuple(_ffi.SERIES_SYMBOLS) == SERIES_SYMBOLS_1
    assert tuple(_ffi.CENSUS_SYMBOLS) == CENSUS_SYMBOLS_1
    assert tuple(_ffi.ROLL_SYMBOLS) == ROLL_SYMBOLS_1
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in ABI_SYMBOLS_15)
    older = set(_ffi.ABI_SYMBOLS) | set(_ffi.TRACK_SYMBOLS) | set(_ffi.SERIES_SYMBOLS) | set(_ffi.CENSUS_SYMBOLS) | set(_ffi.ROLL_SYMBOLS)
    assert not set(_ffi.LEDGER_SYMBOLS) & older
    lib = serf_amd.load()
    assert lib.abi_version() == 15 and oracle.abi_version() == 15
    assert lib.track_version() == 1 and lib.series_version() == 1 and lib.census_version() == 1 and lib.roll_version() == 1
    assert not oracle.has_ledger and oracle.ledger_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.LEDGER_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)
    o = _ffi.Sim(oracle, _ffi.make_config(64))
    e = [(_ffi.K_JOIN, 1, 1)]
    for call in (lambda: o.ledger_start(e), o.ledger_count, o.ledger_read, o.ledger_stop, lambda: o.ledger_now(e)):
        with pytest.raises(NotImplementedError):
            call()


def test_ledger_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "serf_sim_ledger.h"\n'
                    'int main(void){printf("%zu %zu %zu %u %u %u %u %u %u\\n",sizeof(sim_ledger_entry),offsetof(sim_ledger_entry,key),'
                    "offsetof(sim_ledger_entry,val),SIM_LEDGER_MAX,SIM_LEDGER_MAX_SAMPLES,SIM_LEDGER_VERSION,SIM_LEDGER_HEADER_WORDS,"
                    "SIM_LEDGER_ENTRY_WORDS,SIM_CONV_MAX);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_ffi.LedgerEntry), _ffi.LedgerEntry.key.offset, _ffi.LedgerEntry.val.offset, _ffi.LEDGER_MAX,
                   _ffi.LEDGER_MAX_SAMPLES, 1, _ffi.LEDGER_HEADER_WORDS, _ffi.LEDGER_ENTRY_WORDS, 64]
    assert got[:4] == [16, 4, 8, 64]
    # a sample is 8 + 8 n words; the records' fields are the tables' words, in order
    assert _ffi.LEDGER_HEADER_DTYPE.itemsize == _ffi.LEDGER_ENTRY_DTYPE.itemsize == 64
    off = {n: _ffi.LEDGER_HEADER_DTYPE.fields[n][1] // 8 for n in _ffi.LEDGER_HEADER_DTYPE.names}
    assert off == dict(tick=0, running=1, n=2, queued=3, in_flight=4, packets=5, transmits=6, reserved=7)
    off = {n: _ffi.LEDGER_ENTRY_DTYPE.fields[n][1] // 8 for n in _ffi.LEDGER_ENTRY_DTYPE.names}
    assert off == dict(id=0, val=1, reach=2, holders=3, queued=4, transmits=5, in_flight=6, fresh=7)
    for n in (1, 5, 64):
        hdr, rec = _ffi.ledger_split(np.arange(3 * (8 + 8 * n), dtype=np.uint64), n)
        assert hdr.shape == (3,) and rec.shape == (3, n) and hdr["tick"].tolist() == [0, 8 + 8 * n, 2 * (8 + 8 * n)]
        assert rec["fresh"][1, n - 1] == 2 * (8 + 8 * n) - 1


# ---- ledger_summary on hand-made arrays ----
def hand_made(ticks, cols):
    """cols: per entry a dict of field -> list per sample."""
    hdr = np.zeros(len(ticks), _ffi.LEDGER_HEADER_DTYPE)
    hdr["tick"], hdr["running"], hdr["n"] = ticks, 10, len(cols)
    rec = np.zeros((len(ticks), len(cols)), _ffi.LEDGER_ENTRY_DTYPE)
    for i, c in enumerate(cols):
        rec["id"][:, i], rec["val"][:, i] = c["key"] | (c["kind"] << 32), c["val"]
        for f in ("reach", "queued", "in_flight"):
            rec[f][:, i] = c[f]
    return hdr, rec


def test_ledger_summary_on_hand_made_arrays():
    ticks = [5, 6, 7, 8, 9, 10]
    hdr, rec = hand_made(ticks, [
        dict(kind=3, key=0x77, val=4, reach=[0, 1, 4, 8, 9, 9], queued=[0, 1, 3, 4, 1, 0], in_flight=[0, 3, 9, 12, 3, 0]),    # dies at 9, short of 10
        dict(kind=2, key=5, val=7, reach=[0, 0, 0, 2, 6, 10], queued=[0, 0, 0, 2, 4, 4], in_flight=[0, 0, 0, 0, 6, 12]),      # still carried at the end
        dict(kind=6, key=5, val=0, reach=[0] * 6, queued=[0] * 6, in_flight=[0] * 6),                                          # never seen
        dict(kind=3, key=0x78, val=4, reach=[10] * 6, queued=[0] * 6, in_flight=[0, 0, 2, 0, 0, 0])])                           # known to all before the first sample
    s = _ffi.ledger_summary(hdr, rec)
    assert s[0] == dict(kind=3, key=0x77, val=4, first_tick=6, reach=9, running=10, copies=27, died_at=9, reach_at_death=9, copies_per_node=3.0)
    assert s[1] == dict(kind=2, key=5, val=7, first_tick=8, reach=10, running=10, copies=18, died_at=None, reach_at_death=None, copies_per_node=1.8)
    assert s[2] == dict(kind=6, key=5, val=0, first_tick=None, reach=0, running=10, copies=0, died_at=None, reach_at_death=None, copies_per_node=None)
    assert s[3]["first_tick"] == 5 and s[3]["died_at"] == 7 and s[3]["reach_at_death"] == 10 and s[3]["copies"] == 2
    assert _ffi.ledger_summary(hdr[:0], rec[:0]) == []             # (no sample: nothing to say about an entry's course)
