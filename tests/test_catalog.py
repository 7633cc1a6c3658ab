"""Rumour catalogue (include/serf_sim_catalog.h), the part that needs no GPU: the reference model (tests/catalog_model.py)
against the ledger model and the series model on the oracle, the extension's interface, and the conditions of the scenarios
that tests/test_catalog_gpu.py runs on the GPU as well.

This file owns those scenarios.  A scenario is (nodes, configuration, a script drive(sim, step) that injects every operation
up front, the catalogue's start arguments); run() is the script on a fresh oracle with a CatalogModel behind the ticks, once
per session.

  ledger's       dies / lives / twice / census (krandomnodes, bijection) / deep of tests/test_ledger.py, every tick, all kinds
  members        deep with kinds_mask restricted to ALIVE / SUSPECT / DEAD
  two accusers   deep's image with two SUSPECT records about one subject from two accusers written into one queue (two_accusers)
  256 / 257      4 096 nodes, SWIM off, fan-out 1, loss 0.9, retransmit_mult 1: a record leaves its origin's queue after four
                 transmits and nine packets in ten are lost — user events with distinct keys from distinct nodes stay where they
                 were injected long enough to be counted: 256 in tick 2, or 200 in tick 2 and 57 more in tick 4
  registry       256 nodes, max_ids 8, 12 events, four a tick in ticks 2, 3, 4
  crash          64 nodes, loss 1.0: an event that only its origin ever holds; the origin crashes in tick 4 and is back in tick 7
  shapes         the ragged script of tests/test_observer_shapes.py at 64, 65, 257, 4 097 (17 tables: one merge level) and 8 257
                 nodes (33 tables: two levels, the second group of the first level holds ONE table), its idle script, its
                 second pass

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
from tests import test_ledger as tl
from tests import test_observer_shapes as shapes
from tests._oracle import load_oracle
from tests.catalog_model import CatalogModel, identity, live_set, stateless_sample
from tests.ledger_model import sample as ledger_sample
from tests.series_model import sample as series_sample
from tests.test_track_gpu import KRANDOM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATALOG_HEADER = os.path.join(ROOT, "include", "serf_sim_catalog.h")
CATALOG_INC = os.path.join(ROOT, "serf_amd", "csrc", "serf_sim_catalog.inc")
ALL, MEMBERS = _ffi.CATALOG_KINDS, _ffi.catalog_mask((_ffi.K_ALIVE, _ffi.K_SUSPECT, _ffi.K_DEAD))
BLOCK, FANIN = 256, 32                      # serf_sim.hip: #define BLOCK 256; serf_sim_catalog.inc: #define CAT_FANIN 32u


def entry_of(ident):
    """(id, val) -> the ledger's (kind, key, val)."""
    return ident[0] >> 32, ident[0] & 0xFFFFFFFF, ident[1]


# ---- scenarios ----
def none(spec):
    return None


OVER_N = 4096
OVER_KW = dict(fanout=1, retransmit_mult=1, loss=0.9, view_slots=0, event_ring=64, query_ring=64, flags=KRANDOM)
OVER_TICKS = 24


def over_origins(count):
    rng = np.random.default_rng(256)
    return rng.choice(OVER_N, count, replace=False).tolist()


def over_drive(first, second):
    """`first` events in tick 2, `second` more in tick 4, each from a node of its own."""
    def drive(sim, step):
        for i, node in enumerate(over_origins(first + second)):
            sim.inject(2 if i < first else 4, _ffi.OP_USER_EVENT, node, 0x54000000 + i, 64)
        step(OVER_TICKS)
    return drive


REG_N, REG_MAX, REG_TICKS = 256, 8, 30
REG_KW = dict(fanout=3, view_slots=0, event_ring=64, query_ring=64, flags=KRANDOM)


def registry_drive(sim, step):
    for i in range(12):
        sim.inject(2 + i // 4, _ffi.OP_USER_EVENT, 11 * i + 3, 0x55000100 - i, 64)      # (keys descend: rank order is not injection order)
    step(REG_TICKS)


CRASH_N, CRASH_NODE, CRASH_KEY, CRASH_TICKS = 64, 21, 0x56000001, 16
CRASH_KW = dict(fanout=2, loss=1.0, view_slots=0, event_ring=64, query_ring=64, flags=KRANDOM)


def crash_drive(sim, step):
    sim.inject(2, _ffi.OP_USER_EVENT, CRASH_NODE, CRASH_KEY, 64)
    sim.inject(4, _ffi.OP_CRASH, CRASH_NODE)
    sim.inject(7, _ffi.OP_REVIVE, CRASH_NODE)
    step(CRASH_TICKS)


SHAPE_SIZES = (64, 65, 257, 4097, 8257)
SHAPE_TICKS = {4097: 40, 8257: 40}


def ragged_kw(n, fan):
    return shapes.ragged_kw(n, fan)


def ragged_drive(n):
    return lambda sim, step: shapes.ragged_script(sim, n, none, step, SHAPE_TICKS.get(n, shapes.RAGGED_TICKS))


def idle_drive(n):
    return lambda sim, step: shapes.idle_script(sim, n, none, step)


def big_drive(sim, step):
    shapes.big_start(sim, shapes.SERIES_N)
    step(shapes.SERIES_TICKS)


def scenario(name, arg=None):
    """(nodes, configuration, drive, the catalogue's start arguments)."""
    start = dict(kinds_mask=ALL, max_ids=_ffi.CATALOG_MAX, first_tick=0, period=1, capacity=1 << 10)
    if name == "dies":
        return tl.N, tl.DIES_KW, tl.dies_drive, start
    if name == "lives":
        return tl.N, tl.LIVES_KW, tl.dies_drive, start
    if name == "census":
        return tl.N, tl.census_kw(arg), tl.census_ledger_drive, start
    if name == "twice":
        return tl.TWICE_N, tl.TWICE_KW, tl.twice_drive, start
    if name == "deep":
        return tl.DEEP_N, tl.DEEP_KW, tl.deep_drive, start
    if name == "members":
        return tl.DEEP_N, tl.DEEP_KW, tl.deep_drive, dict(start, kinds_mask=MEMBERS)
    if name == "over":
        return OVER_N, OVER_KW, over_drive(*arg), start
    if name == "registry":
        return REG_N, REG_KW, registry_drive, dict(start, max_ids=REG_MAX)
    if name == "crash":
        return CRASH_N, CRASH_KW, crash_drive, start
    if name == "ragged":
        return arg[0], ragged_kw(*arg), ragged_drive(arg[0]), start
    if name == "idle":
        return arg[0], dict(shapes.KW, view_slots=0, flags=shapes.FANOUTS[arg[1]]), idle_drive(arg[0]), start
    if name == "second_pass":
        return shapes.SERIES_N, shapes.BIG_KW, big_drive, dict(start, period=shapes.SERIES_PERIOD)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def run(name, arg=None):
    """Once per session; nobody changes what it returns: dict(oracle, samples, registry, live, now) — `now` the stateless
    sample and live table of the final state."""
    n, kw, drive, start = scenario(name, arg)
    o = tl.maker(n, kw)()
    m = CatalogModel(o)
    m.start(**start)
    drive(o, m.step)
    return dict(oracle=o, samples=m.read(), registry=m.list(), live=m.live(), now=m.now(start["kinds_mask"]), count=m.count())


def tables(n):
    """Slabs the scan writes, and what each merge level leaves."""
    g = min(-(-n // BLOCK), 1024)
    levels = [g]
    while levels[-1] > 1:
        levels.append(-(-levels[-1] // FANIN))
    return levels


# ---- 1. the model against the ledger model and the series model ----
def test_the_model_equals_the_ledger_model_and_the_series_model_at_every_tick():
    """deep: 512 nodes, deep queues, two pages, all seven kinds.  For every identity the model finds, holders, queued,
    transmits, in flight and fresh are the ledger model's words 3-7 of that entry; words 9-12 are its header's 3-6; the
    by-kind in-flight words are the series model's 41-47."""
    o = tl.maker(tl.DEEP_N, tl.DEEP_KW)()
    tl.sc.apply_schedule(o, tl.sc.schedule(tl.DEEP_N, 40, rate=2.0, seed=524, max_member_subjects=40))
    kinds_seen, most = set(), 0
    for _ in range(tl.DEEP_TICKS):
        o.step(1)
        w, table = stateless_sample(o)
        assert not w[3] and w[2] == len(table)
        found = [(int(r["id"]), int(r["val"])) for r in table]
        assert found == sorted(found) and len(set(found)) == len(found)
        hdr = None
        for at in range(0, len(found), _ffi.LEDGER_MAX):
            chunk = [entry_of(x) for x in found[at:at + _ffi.LEDGER_MAX]]
            hdr, rec = _ffi.ledger_split(ledger_sample(o, chunk), len(chunk))
            for f in ("holders", "queued", "transmits", "in_flight", "fresh"):
                assert rec[f][0].tolist() == table[f][at:at + len(chunk)].tolist(), f
            assert ((rec["queued"][0] > 0) | (rec["in_flight"][0] > 0)).all(), "an identity that is not live"
        if hdr is not None:
            assert [int(x) for x in w[9:13]] == [int(hdr[f][0]) for f in ("queued", "in_flight", "packets", "transmits")]
        ser = series_sample(o)
        assert w[27:34].tolist() == [int(x) for x in ser[41:48]] and int(w[9]) == int(ser[6:10].sum()) and int(w[11]) == int(ser[40])
        assert int(w[20:27].sum()) == int(w[9]) and int(w[13:20].sum()) == len(found)
        kinds_seen |= {x[0] >> 32 for x in found}
        most = max(most, len(found))
    assert kinds_seen == set(range(1, 8)) and 64 < most <= _ffi.CATALOG_LIVE
    o.close()


TWO_TICKS = 12     # ticks behind the restore of two_accusers()


@functools.lru_cache(maxsize=None)
def two_accusers():
    """Two SUSPECT records about ONE subject at ONE incarnation from two accusers in ONE queue.  queue_broadcast never leaves
    that behind — a memberlist broadcast invalidates the queued ones about the same node — so the state is made: `deep` on the
    oracle up to the first tick at which some node queues two SUSPECT records (about two subjects), its image, and in the
    image's queue section both records rewritten to a subject nobody has a record about, incarnation 0, accusers 3 and 4.
    Kind, flags, length, transmits and sequence stay: the queue's order holds.  Returns (image, sim_tick, node, subject)."""
    o = tl.maker(tl.DEEP_N, tl.DEEP_KW)()
    tl.sc.apply_schedule(o, tl.sc.schedule(tl.DEEP_N, 40, rate=2.0, seed=524, max_member_subjects=40))
    for _ in range(tl.DEEP_TICKS):
        o.step(1)
        q = o.dump(_ffi.ARR_QUEUE).reshape(tl.DEEP_N, -1)
        sus = (((q["meta"].astype(np.int64) >> 4) & 0xF) == _ffi.K_SUSPECT) & (q["meta"] != 0xFFFFFFFF)
        if sus.sum(axis=1).max() >= 2:
            break
    else:
        raise AssertionError("no node ever queues two SUSPECT records")
    node = int(np.argmax(sus.sum(axis=1)))
    used = set(q["key"][q["meta"] != 0xFFFFFFFF].tolist()) | set(o.dump(_ffi.ARR_INBOX)["key"].reshape(-1).tolist())
    subject = max(x for x in range(tl.DEEP_N) if x not in used)
    image = o.snapshot()
    raw = image.tobytes()
    at = raw.find(q.tobytes())
    assert at >= 0 and raw.count(q.tobytes()) == 1, "the image no longer holds the queues as SIM_ARR_QUEUE dumps them"
    patched = q.copy()
    for accuser, slot in zip((3, 4), np.nonzero(sus[node])[0][:2].tolist()):
        patched["key"][node, slot], patched["val"][node, slot] = subject, accuser << 32
    image = np.frombuffer(raw[:at] + patched.tobytes() + raw[at + q.nbytes:], np.uint8).copy()
    tick = o.tick
    o.close()
    return image, tick, node, subject


@functools.lru_cache(maxsize=None)
def two_accusers_run():
    """The made state restored into a fresh oracle, a catalogue behind TWO_TICKS more ticks: (oracle, the stateless sample and
    table right behind the restore, samples, registry, live)."""
    image, tick, node, subject = two_accusers()
    o = tl.maker(tl.DEEP_N, tl.DEEP_KW)()
    o.restore(image)
    m = CatalogModel(o)
    first = m.now()
    m.start()
    m.step(TWO_TICKS)
    return o, first, m.read(), m.list(), m.live()


def test_two_accusers_in_one_queue_are_one_identity():
    image, tick, node, subject = two_accusers()
    o, (w, table), samples, reg, _ = two_accusers_run()
    ident = (subject | (_ffi.K_SUSPECT << 32), 0)
    at = [(int(r["id"]), int(r["val"])) for r in table].index(ident)
    assert (int(table["holders"][at]), int(table["queued"][at]), int(table["in_flight"][at])) == (1, 2, 0)
    assert w["tick"] == tick and samples["tick"][0] == tick + 1
    rec = reg[[(int(x["id"]), int(x["val"])) for x in reg].index(ident)]
    assert rec["peak_queued"] > rec["peak_holders"] >= 1, "the two records travel on: still one identity"


def test_identity_drops_the_accuser_and_keeps_48_bits():
    assert identity(_ffi.K_SUSPECT, 9, 5 | (77 << 32)) == identity(_ffi.K_SUSPECT, 9, 5 | (3 << 32)) == (9 | (6 << 32), 5)
    assert identity(_ffi.K_DEAD, 9, 5 | (77 << 32))[1] == 5 and identity(_ffi.K_ALIVE, 9, (1 << 50) | 7) == (9 | (5 << 32), 7)
    assert identity(_ffi.K_EVENT, 0x77, (1 << 48) - 1)[1] == (1 << 48) - 1


# ---- 2. the conditions the GPU tests rely on ----
def test_the_ledger_scenarios_on_the_oracle():
    r = run("dies")
    s, reg = r["samples"], r["registry"]
    assert s["tick"].tolist() == list(range(1, tl.DIES_TICKS + 1)) and not s["overflow"].any()
    want = {identity(*e) for e in tl.dies_oracle(True)[1]}
    assert {(int(x["id"]), int(x["val"])) for x in reg} == want and s["new"].sum() == tl.DIES_EVENTS and s["live"][-1] == 0
    assert s["died"].sum() == tl.DIES_EVENTS + s["revived"].sum() and (reg["last_seen"] < tl.DIES_TICKS).all()
    # the registry's sums are the ledger's columns
    _, entries, (hdr, rec) = tl.dies_oracle(True)
    for i, e in enumerate(entries):
        x = reg[[k for k in range(len(reg)) if (int(reg["id"][k]), int(reg["val"][k])) == identity(*e)][0]]
        assert int(x["in_flight_sum"]) == int(rec["in_flight"][:, i].sum()) and int(x["queued_sum"]) == int(rec["queued"][:, i].sum())
        assert int(x["peak_queued"]) == int(rec["queued"][:, i].max()) and int(x["peak_holders"]) == int(rec["holders"][:, i].max())
        assert int(x["peak_queued_at"]) == 1 + int(np.argmax(rec["queued"][:, i]))
    r = run("lives")
    assert (r["registry"]["in_flight_sum"] == 16 * tl.N).all() and len(r["registry"]) == tl.DIES_EVENTS


def test_identities_that_differ_in_val_only_are_live_at_once():
    """twice: one event key at two Lamport times, one subject suspected at two incarnations — a table that compared ids alone
    would fold each pair into one place."""
    r = run("twice")
    s, reg = r["samples"], r["registry"]
    ids = reg["id"].tolist()
    pairs = [i for i in set(ids) if ids.count(i) == 2]
    assert sorted(int(i) >> 32 for i in pairs) == [_ffi.K_EVENT, _ffi.K_SUSPECT] and not s["overflow"].any()
    for i in pairs:
        a, b = [x for x in reg if int(x["id"]) == i]
        assert a["val"] != b["val"] and max(a["first_seen"], b["first_seen"]) < min(a["last_seen"], b["last_seen"]), "never live at once"


@pytest.mark.parametrize("variant", ("krandomnodes", "bijection"))
def test_the_census_scenarios_find_what_nobody_named(variant):
    r = run("census", variant)
    s, reg = r["samples"], r["registry"]
    kinds = {int(x) >> 32 for x in reg["id"]}
    assert {_ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY, _ffi.K_SUSPECT, _ffi.K_DEAD, _ffi.K_ALIVE} <= kinds
    assert len(s) == tl.CENSUS_TICKS and not s["overflow"].any() and s["live"].max() >= 6 and s["ids_lost"][-1] == 0
    assert s["registry"][-1] == len(reg) == s["new"].sum() > 40 and s["revived"].sum() > 0
    assert (reg["val"][(reg["id"] >> np.uint64(32)) == _ffi.K_ALIVE] > 0).any(), "no refuting ALIVE: an incarnation nobody outside knows"


def test_deep_and_its_member_kinds():
    every, members = run("deep"), run("members")
    s, ms = every["samples"], members["samples"]
    assert not s["overflow"].any() and s["live"].max() > 64 and (s["live_by_kind"].max(axis=0) > 0).all()
    assert {int(x) >> 32 for x in members["registry"]["id"]} == {5, 6, 7} and len(members["registry"]) > 8
    assert [c for c in ("queued", "in_flight", "packets", "transmits") if ms[c].tolist() != s[c].tolist()] == []     # words 9-12 cover everything
    assert ms["live_by_kind"][:, 4:].tolist() == s["live_by_kind"][:, 4:].tolist() and not ms["live_by_kind"][:, :4].any()
    assert (ms["queued_by_kind"].sum(axis=1) < ms["queued"]).any()
    keep = [x for x in every["registry"] if int(x["id"]) >> 32 >= 5]
    assert [tuple(x) for x in keep] == [tuple(x) for x in members["registry"]]
    live = every["live"]
    sus = every["samples"]  # (the two-accusers condition: test_the_model_equals_... above)
    assert len(live) == s["live"][-1] and sus["tick"][-1] == tl.DEEP_TICKS


def test_the_overflow_boundary_is_where_it_is_claimed():
    r = run("over", (256, 0))
    s = r["samples"]
    assert not s["overflow"].any() and s["live"][2] == 256 == s["new"][2] and s["live"].max() == 256 and s["overflowed"][-1] == 0
    assert r["oracle"].cluster_stats()["overflow"] == 0
    r = run("over", (200, 57))
    s, o = r["samples"], r["oracle"]
    assert o.cluster_stats()["overflow"] == 0
    assert s["live"][:5].tolist() == [0, 0, 200, 200, 0] and s["overflow"][:6].tolist() == [0, 0, 0, 0, 1, 0]
    # the true count behind tick 4 (sim_tick 5) is 257, one more than a sample holds
    m = tl.maker(OVER_N, OVER_KW)()
    over_drive(200, 57)(m, lambda k: m.step(5))
    assert len(live_set(m)[0]) == 257
    m.close()
    bad = np.nonzero(s["overflow"])[0]
    good = int(bad[-1]) + 1
    assert good < len(s) and 0 < s["live"][good] <= 256 and s["overflowed"][-1] == len(bad)
    for c in ("live", "new", "died", "revived"):
        assert not s[c][bad].any()
    assert (s["registry"][bad] == 200).all() and (s["queued"][bad] > 0).all() and (s["in_flight"][bad] > 0).all()
    # died against the last good sample (200 live behind tick 3), new = the later events that still live
    assert s["died"][good] > 0 and s["died"][good] + s["live"][good] == 200 + s["new"][good] and s["new"][good] > 0


def test_a_full_registry_keeps_the_first_eight():
    r = run("registry")
    s, reg = r["samples"], r["registry"]
    assert len(reg) == REG_MAX and s["ids_lost"][-1] == 4 and s["registry"][-1] == REG_MAX
    assert s["new"][:5].tolist() == [0, 0, 4, 4, 0] and s["ids_lost"][:6].tolist() == [0, 0, 0, 0, 4, 4] and s["live"][4] == 12
    keys = [int(x) & 0xFFFFFFFF for x in reg["id"]]
    assert keys == [0x55000100 - i for i in (3, 2, 1, 0, 7, 6, 5, 4)], "sample by sample, ascending within a sample"
    assert reg["first_seen"].tolist() == [3] * 4 + [4] * 4


def test_crash_and_revive():
    r = run("crash")
    s, reg = r["samples"], r["registry"]
    assert len(reg) == 1 and int(reg["id"][0]) == CRASH_KEY | (_ffi.K_EVENT << 32)
    assert s["live"][:9].tolist() == [0, 0, 1, 1, 0, 0, 0, 1, 0] and s["died"][4] == 1 == s["died"][8] and s["revived"][7] == 1 and s["new"][2] == 1
    assert reg["revivals"][0] == 1 and reg["first_seen"][0] == 3 and reg["peak_holders"][0] == 1
    assert s["running"][4] == CRASH_N - 1 and s["running"][7] == CRASH_N


@pytest.mark.parametrize("n", SHAPE_SIZES)
def test_the_shapes_are_the_ones_claimed(n):
    assert tables(64) == [1] and tables(65) == [1] and tables(257) == [2, 1] and tables(4097) == [17, 1]
    assert tables(8257) == [33, 2, 1] and tables(shapes.SERIES_N) == [1024, 32, 1]
    r = run("ragged", (n, "krandomnodes"))
    s = r["samples"]
    assert not s["overflow"].any() and s["live"].max() >= 3 and s["running"][0] == n > s["running"][-1]
    assert s["queued"].max() > n // 2, "a rumour that most nodes hold at once: every table has it"


def test_the_source_says_what_the_tests_assume():
    src = open(CATALOG_INC).read()
    assert re.search(r"^#define CATALOG_GRID 1024u\b", src, re.M) and re.search(r"^#define CAT_FANIN %du\b" % FANIN, src, re.M)
    assert re.search(r"^#define BLOCK %d$" % BLOCK, open(os.path.join(ROOT, "serf_amd", "csrc", "serf_sim.hip")).read(), re.M)
    for word in ("atomicCAS", "atomicExch", "__hip_atomic"):
        assert word not in src
    assert set(re.findall(r"atomic\w+\(&?(\w+)", src)) == {"hdr", "kinds", "cnt"}, "atomics on the __shared__ arrays only"


# ---- the interface ----
def catalog_declared():
    src = re.sub(r"/\*.*?\*/", "", open(CATALOG_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_catalog_header_declares_what_the_binding_binds():
    assert catalog_declared() == sorted("sim_" + s for s in _ffi.CATALOG_SYMBOLS) and len(_ffi.CATALOG_SYMBOLS) == 8


def test_hip_library_exports_the_catalogue():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in catalog_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    assert lib.has_catalog and lib.catalog_version() == 1


def test_the_oracle_has_no_catalogue(oracle):
    assert not oracle.has_catalog and oracle.catalog_version() is None
    o = _ffi.Sim(oracle, _ffi.make_config(64))
    for call in (o.catalog_start, o.catalog_count, o.catalog_read, o.catalog_stop, o.catalog_list, o.catalog_live, o.catalog_now):
        with pytest.raises(NotImplementedError):
            call()
    o.close()


def test_catalog_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include "serf_sim_catalog.h"\n'
                    'int main(void){printf("%u %u %u %u %u %u %u\\n",SIM_CATALOG_VERSION,SIM_CATALOG_LIVE,SIM_CATALOG_MAX,'
                    "SIM_CATALOG_MAX_SAMPLES,SIM_CATALOG_SAMPLE_WORDS,SIM_CATALOG_RECORD_WORDS,SIM_CATALOG_KINDS);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [1, _ffi.CATALOG_LIVE, _ffi.CATALOG_MAX, _ffi.CATALOG_MAX_SAMPLES, _ffi.CATALOG_SAMPLE_WORDS, _ffi.CATALOG_RECORD_WORDS,
                   _ffi.CATALOG_KINDS] == [1, 256, 4096, 1 << 20, 48, 8, 0xFE]
    off = {n: _ffi.CATALOG_SAMPLE_DTYPE.fields[n][1] // 8 for n in _ffi.CATALOG_SAMPLE_DTYPE.names}
    assert off == dict(tick=0, running=1, live=2, overflow=3, new=4, died=5, revived=6, registry=7, ids_lost=8, queued=9, in_flight=10,
                       packets=11, transmits=12, live_by_kind=13, queued_by_kind=20, in_flight_by_kind=27, overflowed=34, reserved=35)
    assert list(_ffi.CATALOG_LIVE_DTYPE.names) == ["id", "val", "reserved"] + list(_ffi.LEDGER_ENTRY_DTYPE.names[3:])
    rec = np.zeros(1, _ffi.CATALOG_RECORD_DTYPE)
    rec.view(np.uint64)[:] = [1, 2, 3 | (4 << 32), 5 | (6 << 32), 7 | (8 << 32), 9 | (10 << 32), 11, 12]
    assert [int(x) for x in rec[0]] == list(range(1, 13))
    assert _ffi.catalog_mask(range(1, 8)) == _ffi.CATALOG_KINDS and MEMBERS == 0xE0


def test_catalog_summary_on_a_model_registry():
    reg = run("registry")["registry"]
    s = _ffi.catalog_summary(reg)
    assert [d["key"] for d in s["identities"]] == [int(x) & 0xFFFFFFFF for x in reg["id"]] and list(s["by_kind"]) == [_ffi.K_EVENT]
    k = s["by_kind"][_ffi.K_EVENT]
    assert k["identities"] == REG_MAX and k["copies"] == int(reg["in_flight_sum"].sum())
    assert k["longest_life"] == int((reg["last_seen"] - reg["first_seen"]).max()) + 1
    assert _ffi.catalog_summary(reg[:0]) == dict(identities=[], by_kind={})
