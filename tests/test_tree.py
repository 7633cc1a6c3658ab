"""Rumour tree (include/serf_sim_tree.h), the part that needs no GPU: the reference model (tests/tree_model.py) on the CPU oracle
against routes that do not share its code — the spread map's arrivals, the ledger's copies in flight, the kRandomNodes draw of
every parent, the traffic meter's tx_packets —, the invariants of a tree, the conditions that make the scenarios non-trivial,
the stamp rule, and the extension's interface next to the ABI and the eight extensions it must not disturb.

This file owns the scenarios tests/test_tree_gpu.py drives the HIP library through.  Everything compared is an exact integer."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from serf_amd.workload import apply_schedule
from tests import ledger_model, test_abi
from tests import test_spread as tsp
from tests import test_traffic as tt
from tests.spread_model import SpreadModel
from tests.third_model import k_random_nodes
from tests.traffic_model import TrafficModel
from tests.tree_model import TreeModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_HEADER = os.path.join(ROOT, "include", "serf_sim_tree.h")
TREE_INC = os.path.join(ROOT, "serf_amd", "csrc", "serf_sim_tree.inc")
TREE_GRID = 1024                          # serf_sim_tree.inc: #define TREE_GRID 1024u; per_pass = gridDim.x * BLOCK
NONE = _ffi.TREE_NONE
FANOUTS, FANOUT = tt.FANOUTS, tt.FANOUT
SPREAD_SYMBOLS_1 = ("spread_start", "spread_count", "spread_read", "spread_stop", "spread_map", "spread_summary", "spread_unreached",
                    "spread_late", "spread_version")
TRAFFIC_SYMBOLS_1 = ("traffic_start", "traffic_count", "traffic_read", "traffic_stop", "traffic_nodes", "traffic_top", "traffic_summary",
                     "traffic_version")
NEVER = (_ffi.K_EVENT, 0x7ABCDEF, 3)      # an entry nobody ever injects


# ---- the scenarios ----
def quiet_kw(n, fan, **more):
    """No SWIM layer, no push-pull: packets are the only way a rumour travels."""
    return dict(dict(fanout=FANOUT, view_slots=0 if n <= 65 else 16, event_ring=64, query_ring=64, flags=FANOUTS[fan], probe_interval=0,
                     push_pull_interval=0), **more)


def inject_events(sim, origins, key0=0x7700):
    """One user event per origin into the state `sim` is in; returns their entries."""
    entries = []
    for i, x in enumerate(origins):
        entries.append((_ffi.K_EVENT, key0 + i, int(sim.stats(x).event_time)))
        sim.user_event(x, key0 + i, 64)
    return entries


QUIET = {  # name -> (nodes, fan-out model, more configuration, the events' origins, ticks)
    "65": (65, None, {}, (5, 40), 16),
    "257": (257, None, {}, (5,), 25),
    "257_loss": (257, None, dict(loss=0.3), (5, 100, 200), 30),
}
SWIM_N, SWIM_TICKS = 1000, 30
SWIM_KW = dict(loss=0.1, probe_interval=5, push_pull_interval=4, view_slots=32)


@functools.lru_cache(maxsize=None)
def quiet_run(name, fan):
    """Started at tick 0 before the events are injected.  dict(o, m, entries, per tick: the spread model's arrivals, the ledger
    model's words, the traffic model's map)."""
    n, _, more, origins, ticks = QUIET[name]
    o = tt.make(n, quiet_kw(n, fan, **more))
    entries = inject_events(tt.make(n, quiet_kw(n, fan, **more)), origins)      # (a scratch handle: the clocks are those of tick 0)
    spread, ledger, trees = [], [], []
    sm, tm = SpreadModel(o), TrafficModel(o)

    def each():
        sm.after_tick(o.tick - 1)
        tm.after_tick(o.tick - 1)
        spread.append(sm.arrival.copy())
        ledger.append(ledger_model.sample(o, entries))
        trees.append((m.arrival.copy(), m.parent.copy(), m.hop.copy()))
    m = TreeModel(o, each)
    m.start(entries, 0, ticks)
    sm.start(entries, 0, 1, ticks)
    tm.start(0, 1, ticks)
    assert inject_events(o, origins) == entries
    m.step(ticks)
    return dict(o=o, m=m, n=n, entries=entries, spread=spread, ledger=ledger, trees=trees, traffic=tm, ticks=ticks)


@functools.lru_cache(maxsize=None)
def swim_run(fan):
    n = SWIM_N
    kw = tt.churn_kw(n, fan, **SWIM_KW)
    origins = (5, 400, 900)
    entries = inject_events(tt.make(n, kw), origins)
    o = tt.make(n, kw)
    m = TreeModel(o)
    m.start(entries, 0, SWIM_TICKS)
    inject_events(o, origins)
    m.step(SWIM_TICKS)
    return dict(o=o, m=m, n=n, entries=entries)


def tree_ops(n, ticks=tt.CHURN_TICKS, burst=0):
    """tests/test_traffic.py's churn schedule and one rejoin of a running node on top: a JOIN record travels too."""
    ops = tt.churn_ops(n, ticks, burst=burst)
    if n >= 4:
        ops.append((4, _ffi.OP_JOIN, n // 3, 0, 0))
    return sorted(ops, key=lambda o: o[0])


@functools.lru_cache(maxsize=None)
def dry_entries(n, kw_items, ops, ticks, events=12):
    """The identities of kinds 1-4 a dry run of a schedule on the oracle shows queued or in flight: user events (`events` at
    most), one JOIN, one LEAVE and one QUERY where the run has them, and one entry that is never injected."""
    o = tt.make(n, dict(kw_items))
    apply_schedule(o, list(ops))
    ids = set()
    for _ in range(ticks):
        o.step(1)
        ids |= {i for i in ledger_model.identities(o) if i[0] <= _ffi.K_QUERY}
        wk, wkey, wval, _ = ledger_model.wire_records(o)
        ids |= {i for i in zip(wk.tolist(), wkey.tolist(), [int(v) for v in wval]) if i[0] <= _ffi.K_QUERY}
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0, "the run stays inside the model's bounds"
    o.close()
    ids = sorted(i for i in ids if i[2] < (1 << 48) and (i[1] != 0 or i[0] <= _ffi.K_LEAVE))
    pick = [i for i in ids if i[0] == _ffi.K_EVENT][:events]
    for kind in (_ffi.K_JOIN, _ffi.K_LEAVE, _ffi.K_QUERY):
        pick += [i for i in ids if i[0] == kind][:1]
    return tuple(pick) + (NEVER,)


def churn_entries(n, fan, ticks=tt.CHURN_TICKS, burst=0, more=()):
    return dry_entries(n, tuple(sorted(tt.churn_kw(n, fan, **dict(more)).items())), tuple(tree_ops(n, ticks, burst=burst)), ticks)


def many_ops(n, k=63, per_tick=7):
    """k user events from k nodes, per_tick a tick from tick 0 on."""
    return [(i // per_tick, _ffi.OP_USER_EVENT, (4 * i + 1) % n, 0x7800 + i, 64) for i in range(k)]


def tree_invariants(m, what=""):
    """What holds of every tree the model (or anyone) builds."""
    s = m.summary()
    for e in range(len(m.entries)):
        lk = m.links(e)
        a, par, hop, ch = (lk[f].astype(np.int64) for f in ("arrival", "parent", "hop", "children"))
        got, child = a != 0, (a != 0) & (par != NONE)
        assert (par[~got] == NONE).all() and not hop[~got].any()
        assert (a[par[child]] > 0).all() and (a[par[child]] < a[child]).all(), f"{what} entry {e}: a parent arrived before its child"
        assert (hop[child] == hop[par[child]] + 1).all() and not hop[got & ~child].any()
        assert ch.sum() == got.sum() - (got & ~child).sum() == child.sum(), "the children sum to reached - orphans"
        assert s["reached"][e] == got.sum() and s["orphans"][e] == (got & ~child).sum() and s["hop_sum"][e] == hop.sum()
        assert s["hop_bins"][e].sum() == s["children_bins"][e].sum() == got.sum() and s["depth"][e] == hop.max(initial=0)
        for node in np.nonzero(got)[0][:: max(1, int(got.sum()) // 7)]:
            ids, total = m.path(e, int(node))
            assert total == len(ids) == hop[node] + 1 and ids[0] == node and par[ids[-1]] == NONE
            assert (par[ids[:-1]] == ids[1:]).all()
        assert m.path(e, int(np.nonzero(~got)[0][0]))[1] == 0 if (~got).any() else True


# ---- 1. the model against other routes ----
@pytest.mark.parametrize("fan", sorted(FANOUTS))
@pytest.mark.parametrize("name", sorted(QUIET))
def test_arrivals_are_the_spread_maps_and_copies_the_ledgers(name, fan):
    run = quiet_run(name, fan)
    hdr, rec = run["m"].read()
    assert hdr["tick"].tolist() == list(range(1, run["ticks"] + 1))
    for t in range(run["ticks"]):
        assert (run["trees"][t][0] == run["spread"][t]).all(), f"tick {t}: arrival is the spread map's plane"
        led = run["ledger"][t]
        assert rec["copies"][t].tolist() == [int(led[8 + 8 * i + 6]) for i in range(len(run["entries"]))], f"tick {t}: the ledger's word 6"
    assert rec["copies"].sum() > 0 and (hdr["copies"] == rec["copies"].sum(axis=1)).all() and (hdr["fresh"] == rec["fresh"].sum(axis=1)).all()
    assert (rec["fresh"] <= rec["copies"]).all(), "one record of an identity a packet here: a carrier is a copy"
    assert rec["new"].sum(axis=0).tolist() == rec["reached"][-1].tolist() and rec["new_orphans"].sum(axis=0).tolist() == rec["orphans"][-1].tolist()
    assert (hdr["new"] == rec["new"].sum(axis=1)).all() and (hdr["new_orphans"] == rec["new_orphans"].sum(axis=1)).all()


@pytest.mark.parametrize("fan", sorted(FANOUTS))
@pytest.mark.parametrize("name", sorted(QUIET))
def test_tree_invariants_and_one_orphan_per_event(name, fan):
    run = quiet_run(name, fan)
    m = run["m"]
    tree_invariants(m, f"{name} {fan}")
    s = m.summary()
    assert s["orphans"].tolist() == [1] * len(run["entries"]), "packets are the only route: the origin alone is an orphan"
    assert (s["depth"] >= 4).all() and (s["reached"] > run["n"] // 2).all()
    if name.startswith("257"):
        assert m.multi > 0, "an arrival had carriers of two different senders: `the smallest sender` decides something"
    hops = _ffi.tree_hops(m.links(0))
    assert hops["reached"] == s["reached"][0] and hops["orphans"] == 1 and hops["depth"] == s["depth"][0] == hops["percentiles"][100]
    assert abs(hops["mean_hop"] * hops["reached"] - int(s["hop_sum"][0])) < 1e-6 and hops["orphan_share"] == 1 / hops["reached"]


@pytest.mark.parametrize("name", sorted(QUIET))
def test_a_child_is_in_its_parents_draw(name):
    """kRandomNodes: the child latched at `arrival` was addressed by a packet sent during tick arrival - 2."""
    run = quiet_run(name, "krandomnodes")
    m, n = run["m"], run["n"]
    seed, links = int(run["o"].cfg.seed), 0
    for e in range(len(run["entries"])):
        lk = m.links(e)
        for child in np.nonzero((lk["arrival"] != 0) & (lk["parent"] != NONE))[0]:
            assert child in k_random_nodes(seed, int(lk["arrival"][child]) - 2, int(lk["parent"][child]), n, FANOUT)
            links += 1
    assert links > n // 2


@pytest.mark.parametrize("fan", sorted(FANOUTS))
def test_children_do_not_exceed_the_packets_sent(fan):
    """One event alone in an idle cluster: every child took one packet of its parent's."""
    run = quiet_run("257", fan)
    ch = run["m"].links(0)["children"]
    assert (ch <= run["traffic"].nodes()["tx_packets"]).all() and ch.max() > 1


@pytest.mark.parametrize("fan", sorted(FANOUTS))
def test_push_pull_makes_orphans(fan):
    run = swim_run(fan)
    tree_invariants(run["m"], f"swim {fan}")
    s = run["m"].summary()
    assert (s["orphans"] > 1).all(), "push-pull delivers without a packet"
    assert (s["depth"] >= 4).all()


@pytest.mark.parametrize("fan", sorted(FANOUTS))
def test_the_churn_schedule_follows_every_kind(fan):
    entries = churn_entries(257, fan)
    kinds = [e[0] for e in entries]
    assert _ffi.K_JOIN in kinds and _ffi.K_LEAVE in kinds and kinds.count(_ffi.K_EVENT) >= 3 and entries[-1] == NEVER
    o = tt.make(257, tt.churn_kw(257, fan))
    apply_schedule(o, tree_ops(257))
    m = TreeModel(o)
    m.start(entries, 0, tt.CHURN_TICKS)
    m.step(tt.CHURN_TICKS)
    tree_invariants(m, f"churn {fan}")
    s = m.summary()
    assert s["reached"][-1] == 0 and (s["reached"][:-1] > 0).all() and (s["reached"] - s["orphans"])[:-1].sum() > 257
    o.close()


def test_the_burst_puts_carriers_behind_the_first_page():
    """What tests/test_tree_gpu.py's pkt_records = 16 run is for: some followed record travels on a page behind the first."""
    n, fan = 257, "krandomnodes"
    entries = churn_entries(n, fan, burst=tt.PKT16_BURST, more=tuple(sorted(tt.PKT16.items())))
    o = tt.make(n, tt.churn_kw(n, fan, **tt.PKT16))
    apply_schedule(o, tree_ops(n, burst=tt.PKT16_BURST))
    later = 0
    for _ in range(10):
        o.step(1)
        inbox = o.dump(_ffi.ARR_INBOX).reshape(-1, n)
        pg = inbox.shape[0] // FANOUT
        kind = ((inbox["hi_meta"].astype(np.int64) >> 4) & 0xF).reshape(FANOUT, pg, n, 4)
        key = inbox["key"].astype(np.int64).reshape(FANOUT, pg, n, 4)
        for k, ky, _ in entries:
            later += int(((kind[:, 1:] == k) & (key[:, 1:] == ky)).sum())
    assert pg == 4 and later > 0
    o.close()


# ---- 2. the sampling rules ----
def test_a_later_start_latches_every_holder_as_an_orphan():
    n, kw = 257, quiet_kw(257, "krandomnodes")
    o = tt.make(n, kw)
    entries = inject_events(o, (5,))
    o.step(3)
    m = TreeModel(o)
    m.start(entries, 1, 30)                      # (a first_tick that has passed: now)
    m.step(1)
    hdr, rec = m.read()
    held = int(rec["reached"][0][0])
    assert hdr["tick"].tolist() == [4] and held > 4 and rec["orphans"][0][0] == held == rec["new_orphans"][0][0], "no sample before it: no candidates"
    m.step(10)
    tree_invariants(m, "a later start")
    s = m.summary()
    assert s["orphans"][0] == held and s["reached"][0] > 2 * held, "behind the first sample the packets name the parents"
    o.close()


def test_the_stamp_rule_across_a_restore():
    """A tree started at tick 0 on a fresh handle that is then restored to tick 2: the first sample behind the restore has no
    candidates of a sample stamped 2 — it latches orphans only."""
    n, kw = 257, quiet_kw(257, "krandomnodes")
    src = tt.make(n, kw)
    entries = inject_events(src, (5,))
    src.step(2)
    img = src.snapshot()
    o = tt.make(n, kw)
    m = TreeModel(o)
    m.start(entries, 0, 30)
    o.restore(img)
    assert o.tick == 2 and m.count() == (0, 0)
    m.step(1)
    hdr, rec = m.read()
    assert hdr["tick"].tolist() == [3] and rec["new"][0][0] == rec["new_orphans"][0][0] > 1
    m.step(1)
    tree_invariants(m, "across a restore")
    assert m.summary()["orphans"][0] == rec["new_orphans"][0][0] < m.summary()["reached"][0]
    # the same when a sample exists but its stamp is not now - 1
    m.stamp -= 1
    before = int(m.summary()["orphans"][0])
    m.step(1)
    assert m.read()[1]["new"][-1][0] == m.read()[1]["new_orphans"][-1][0] > 0 and m.summary()["orphans"][0] > before
    o.close()
    src.close()


def test_a_full_buffer_stops_the_tree():
    n, kw = 65, quiet_kw(65, "bijection")
    o = tt.make(n, kw)
    m = TreeModel(o)
    entries = inject_events(tt.make(n, kw), (5,))
    m.start(entries, 1, 3)
    inject_events(o, (5,))
    m.step(10)
    hdr, rec = m.read()
    assert m.count() == (3, 6) and hdr["tick"].tolist() == [2, 3, 4]
    assert m.summary()["reached"][0] == rec["reached"][-1][0] < n, "a dropped sample latches nothing"
    m.stop()
    assert m.count() == (0, 0)
    o.close()


def test_tree_hops_on_hand_made_links():
    lk = np.zeros(8, _ffi.TREE_LINK_DTYPE)
    lk["arrival"] = [1, 3, 3, 4, 0, 5, 5, 0]
    lk["parent"] = [NONE, 0, 0, 1, NONE, 3, NONE, NONE]
    lk["hop"] = [0, 1, 1, 2, 0, 3, 0, 0]
    h = _ffi.tree_hops(lk, (50, 90, 100))
    assert h == {"reached": 6, "orphans": 2, "orphan_share": 2 / 6, "depth": 3, "mean_hop": 7 / 6, "percentiles": {50: 1, 90: 3, 100: 3}}
    assert _ffi.tree_hops(lk[:0])["percentiles"] == {50: None, 90: None, 99: None, 100: None} and _ffi.tree_hops(lk[:0])["orphan_share"] == 0.0
    with pytest.raises(ValueError):
        _ffi.tree_hops(lk, (0,))


# ---- 3. the interface ----
def tree_declared():
    src = re.sub(r"/\*.*?\*/", "", open(TREE_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t|const char\s*\*)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_tree_header_declares_what_the_binding_binds():
    assert tree_declared() == sorted("sim_" + s for s in _ffi.TREE_SYMBOLS)
    assert len(_ffi.TREE_SYMBOLS) == 9


def test_hip_library_exports_the_tree():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in tree_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    fn = dll.sim_tree_version
    fn.restype = C.c_uint32
    assert fn() == 1
    assert lib.has_tree and lib.tree_version() == 1


def test_the_abi_and_the_eight_older_extensions_are_what_they_were(oracle):
    """The tree is an extension: serf_sim.h, the eight older headers, their symbol lists and the ABI version do not know it; the
    oracle has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == tsp.ABI_SYMBOLS_15
    older = set(_ffi.ABI_SYMBOLS)
    for got, want in ((_ffi.TRACK_SYMBOLS, tsp.TRACK_SYMBOLS_1), (_ffi.SERIES_SYMBOLS, tsp.SERIES_SYMBOLS_1), (_ffi.CENSUS_SYMBOLS, tsp.CENSUS_SYMBOLS_1),
                      (_ffi.ROLL_SYMBOLS, tsp.tl.ROLL_SYMBOLS_1), (_ffi.LEDGER_SYMBOLS, tsp.LEDGER_SYMBOLS_1), (_ffi.DETECT_SYMBOLS, tsp.DETECT_SYMBOLS_1),
                      (_ffi.SPREAD_SYMBOLS, SPREAD_SYMBOLS_1), (_ffi.TRAFFIC_SYMBOLS, TRAFFIC_SYMBOLS_1)):
        assert tuple(got) == want
        older |= set(got)
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in tsp.ABI_SYMBOLS_15)
    assert tsp.spread_declared() == sorted("sim_" + s for s in SPREAD_SYMBOLS_1)
    assert not set(_ffi.TREE_SYMBOLS) & older
    lib = serf_amd.load()
    assert lib.abi_version() == 15 and oracle.abi_version() == 15
    assert [lib.track_version(), lib.series_version(), lib.census_version(), lib.roll_version(), lib.ledger_version(), lib.detect_version(),
            lib.spread_version(), lib.traffic_version()] == [1] * 8
    dll = C.CDLL(lib.path)
    for s in older:
        assert hasattr(dll, "sim_" + s), s
    assert not oracle.has_tree and oracle.tree_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.TREE_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)
    o = _ffi.Sim(oracle, _ffi.make_config(64))
    e = [(_ffi.K_JOIN, 1, 1)]
    for call in (lambda: o.tree_start(e), o.tree_count, o.tree_read, o.tree_stop, lambda: o.tree_links(0), o.tree_summary,
                 lambda: o.tree_path(0, 0), lambda: o.tree_top(0)):
        with pytest.raises(NotImplementedError):
            call()
    o.close()


def test_tree_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "serf_sim_tree.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %u %u %u %u %u %u\\n",sizeof(sim_tree_entry),'
                    "offsetof(sim_tree_entry,key),offsetof(sim_tree_entry,ltime),sizeof(sim_tree_link),offsetof(sim_tree_link,parent),"
                    "offsetof(sim_tree_link,hop),offsetof(sim_tree_link,children),sizeof(sim_tree_rank),offsetof(sim_tree_rank,running),"
                    "offsetof(sim_tree_rank,link),SIM_TREE_MAX,SIM_TREE_MAX_SAMPLES,SIM_TREE_VERSION,SIM_TREE_HEADER_WORDS,SIM_TREE_ENTRY_WORDS,"
                    "SIM_TREE_BINS,SIM_TREE_SUMMARY_WORDS,SIM_TREE_TOP_MAX,SIM_TREE_NONE);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_ffi.SpreadEntry), _ffi.SpreadEntry.key.offset, _ffi.SpreadEntry.ltime.offset, C.sizeof(_ffi.TreeLink),
                   _ffi.TreeLink.parent.offset, _ffi.TreeLink.hop.offset, _ffi.TreeLink.children.offset, C.sizeof(_ffi.TreeRank),
                   _ffi.TreeRank.running.offset, _ffi.TreeRank.link.offset, _ffi.TREE_MAX, _ffi.TREE_MAX_SAMPLES, 1, _ffi.TREE_HEADER_WORDS,
                   _ffi.TREE_ENTRY_WORDS, _ffi.TREE_BINS, _ffi.TREE_SUMMARY_WORDS, _ffi.TREE_TOP_MAX, _ffi.TREE_NONE]
    assert got[:10] == [16, 4, 8, 16, 4, 8, 12, 24, 4, 8] and got[10] == 64
    assert _ffi.TREE_LINK_DTYPE.itemsize == 16 and _ffi.TREE_RANK_DTYPE.itemsize == 24
    off = {n: _ffi.TREE_LINK_DTYPE.fields[n][1] for n in _ffi.TREE_LINK_DTYPE.names}
    assert off == dict(arrival=0, parent=4, hop=8, children=12) and _ffi.TREE_RANK_DTYPE.fields["link"][1] == 8
    off = {n: _ffi.TREE_HEADER_DTYPE.fields[n][1] // 8 for n in _ffi.TREE_HEADER_DTYPE.names}
    assert off == dict(tick=0, running=1, n=2, new=3, new_orphans=4, copies=5, fresh=6, reserved=7)
    off = {n: _ffi.TREE_ENTRY_DTYPE.fields[n][1] // 8 for n in _ffi.TREE_ENTRY_DTYPE.names}
    assert off == dict(id=0, val=1, new=2, new_orphans=3, reached=4, orphans=5, copies=6, fresh=7)
    off = {n: _ffi.TREE_SUMMARY_DTYPE.fields[n][1] // 8 for n in _ffi.TREE_SUMMARY_DTYPE.names}
    assert off == dict(id=0, val=1, reached=2, orphans=3, depth=4, hop_sum=5, most_children=6, most_children_id=7, hop_bins=8, children_bins=40)
    for n in (1, 5, 64):
        hdr, rec = _ffi.tree_split(np.arange(3 * (8 + 8 * n), dtype=np.uint64), n)
        assert hdr.shape == (3,) and rec.shape == (3, n) and rec["fresh"][1, n - 1] == 2 * (8 + 8 * n) - 1


def test_the_cap_is_the_sources():
    """TREE_GRID above mirrors these lines; a change there has to move the second-pass size of tests/test_tree_gpu.py."""
    src = open(TREE_INC).read()
    assert re.search(r"^#define TREE_GRID %du\b" % TREE_GRID, src, re.M)
    assert src.count("const size_t per_pass = (size_t)gridDim.x * BLOCK;") == 3        # the latch, carry and candidate kernels
    assert "p.G = tree_grid(h);" in src and "std::min<size_t>(((size_t)h->d.Nl + BLOCK - 1) / BLOCK, TREE_GRID)" in src
    assert re.search(r"^#define BLOCK 256$", open(os.path.join(ROOT, "serf_amd", "csrc", "serf_sim.hip")).read(), re.M)
    assert re.search(r"OB_TRAFFIC = 6, OB_TREE = 7, OB_N = 8 \}", open(os.path.join(ROOT, "serf_amd", "csrc", "serf_sim_host.inc")).read())
