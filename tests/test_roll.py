"""Observer roll (include/serf_sim_roll.h), the part that needs no GPU: the extension's interface next to the ABI and the three
extensions it must not disturb, and the reference model (tests/roll_model.py) against two independent routes on the oracle
(sim_members per observer, the census model), on scenarios that are asserted to be non-trivial.

This file owns the scenarios that tests/test_roll_gpu.py runs on the GPU as well:

  census     the four scenarios of tests/test_census.py (census_drive, census_kw) at 4 096 nodes, 200 ticks, a roll behind
             every tick, top_k 8; the lossy one ranked three ways
  busy       4 096 nodes, loss 0.03, 26 nodes crash or leave within five ticks and four come back: `stale` reaches 16 and
             more, and thousands of observers tie at the top, so that the id tie-break decides across workgroups
  cold join  64 nodes that start alone and join one per tick: the only scenario with `unknown` > 0
  slots      16 view slots that are recycled while one sim_step(170) runs

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
from tests._oracle import load_oracle
from tests.census_model import sample as census_sample
from tests.roll_model import RollModel, node_records, sample, score_of, split, stale_bin
from tests.test_census import SERIES_SYMBOLS_1, census_drive, census_kw
from tests.test_series import TRACK_SYMBOLS_1, scenario
from tests.test_track import ABI_SYMBOLS_15
from tests.test_track_gpu import KRANDOM, KW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLL_HEADER = os.path.join(ROOT, "include", "serf_sim_roll.h")
CENSUS_SYMBOLS_1 = ("census_start", "census_count", "census_read", "census_stop", "census_now", "census_version")
STALE, ACCUSED, MISSED = _ffi.ROLL_BY_STALE, _ffi.ROLL_BY_ACCUSED, _ffi.ROLL_BY_MISSED
N, TICKS, TOP_K = 4096, 200, 8
VARIANTS = ("krandomnodes", "bijection", "vshards_4", "lossy")


class Ties:
    """Behind every tick a RollModel samples: how many observers share the top score (0 when the top score is 0)."""

    def __init__(self, sim, model):
        self.sim, self.model, self.seen = sim, model, []

    def __call__(self):
        m, t = self.model, self.sim.tick - 1
        if m.running and t >= m.first and (t - m.first) % m.period == 0 and len(self.seen) < m.capacity:
            w, up, _ = node_records(self.sim)
            s = score_of(w, m.rank_by)
            self.seen.append(int((s == s.max()).sum()) if s.max() > 0 else 0)


def models_run(o, specs, script):
    """`script(o, step)` on the oracle with one RollModel per spec (first, period, capacity, top_k, rank_by) behind the ticks.
    Returns (models, ties of the first)."""
    ms = [RollModel(o) for _ in specs]
    ties = Ties(o, ms[0])
    ms[0].on_tick = lambda: ([m.after_tick(o.tick - 1) for m in ms[1:]], ties())
    for m, spec in zip(ms, specs):
        m.start(*spec)
    script(o, ms[0].step)
    return ms, ties.seen


def inside_bounds(o):
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0            # the run stays inside the model's bounds
    return cs


# ---- the census scenarios ----
def census_rank_bys(variant):
    return (STALE, ACCUSED, MISSED) if variant == "lossy" else (STALE,)


@functools.lru_cache(maxsize=None)
def census_oracle(variant):
    """Once per session; nobody changes what it returns: (oracle, {rank_by: (headers, records)}, ties of the STALE roll)."""
    o = _ffi.Sim(load_oracle(), _ffi.make_config(N, **census_kw(variant)))
    bys = census_rank_bys(variant)
    ms, ties = models_run(o, [(0, 1, TICKS, TOP_K, by) for by in bys], lambda sim, step: census_drive(sim, scenario(N), TICKS, step))
    return o, {by: m.read() for by, m in zip(bys, ms)}, ties


def check_census_scenario(variant, run):
    o, reads, ties = run
    inside_bounds(o)
    hdr, rec = reads[STALE]
    assert hdr["tick"].tolist() == list(range(1, TICKS + 1)) and rec.shape == (TICKS, TOP_K)
    assert hdr["stale_max"].max() >= 2 and hdr["accusers_failed"].max() > 0
    # ticks on which the top score is shared, so that the id tie-break decides: 103 of 200 in the lossy variant, 14 to 16 in the
    # others, where fewer observers ever fall behind
    assert sum(1 for t in ties if t > 1) >= (50 if variant == "lossy" else 10)
    assert hdr["lag_max"].max() > 0 and hdr["holders_stale_alive"].max() > 0 and hdr["accusers_suspect"].max() > 0
    for by, (h, r) in reads.items():
        assert ((h["listed"] >> 32) == by).all() and ((h["listed"] & 0xFFFFFFFF) > 0).any()


# ---- busy ----
BUSY_TICKS, BUSY_PERIOD = 80, 4
BUSY_KW = dict(KW, flags=KRANDOM, loss=0.03, recycle_interval=20)


def busy_script(sim, step):
    ids = np.random.default_rng(5).choice(N, 40, replace=False).tolist()
    for i, x in enumerate(ids[0:10]):
        sim.inject(8 + i % 3, _ffi.OP_CRASH, x)
    for i, x in enumerate(ids[10:26]):
        sim.inject(10 + i % 2, _ffi.OP_LEAVE, x)
    for x in ids[0:4]:
        sim.inject(40, _ffi.OP_REVIVE, x)
    step(BUSY_TICKS)


@functools.lru_cache(maxsize=None)
def busy_oracle():
    o = _ffi.Sim(load_oracle(), _ffi.make_config(N, **BUSY_KW))
    (m,), ties = models_run(o, [(0, BUSY_PERIOD, 100, TOP_K, STALE)], busy_script)
    return o, m.read(), ties


def check_busy(run):
    o, (hdr, rec), ties = run
    inside_bounds(o)
    assert len(hdr) == BUSY_TICKS // BUSY_PERIOD and hdr["subjects"].max() <= 64
    assert hdr["stale_max"].max() >= 16
    assert ((hdr["stale_bins"] > 0).sum(axis=1) >= 4).any(), "no tick with four bins in use"
    assert max(ties) > 256, "no tie at the top that spans workgroups"
    i = int(np.argmax(ties))                                          # there the listed ones are the lowest ids of the tied
    ids = (rec[i]["id"] & 0xFFFFFFFF).astype(np.int64)
    assert (rec[i]["stale"] == hdr["stale_max"][i]).all() and (np.diff(ids) > 0).all()


# ---- cold join ----
COLD_N, COLD_TICKS, COLD_TOP = 64, 140, 64
COLD_KW = dict(flags=0, fanout=3, probe_interval=5, loss=0.02, event_ring=64, query_ring=64, push_pull_interval=30)


def cold_script(sim, step):
    for i in range(1, COLD_N):
        sim.inject(1 + i, _ffi.OP_JOIN, i, i // 2)
    sim.inject(100, _ffi.OP_CRASH, 9)
    step(COLD_TICKS)


@functools.lru_cache(maxsize=None)
def cold_oracle():
    o = _ffi.Sim(load_oracle(), _ffi.make_config(COLD_N, **COLD_KW))
    (m,), _ = models_run(o, [(0, 1, COLD_TICKS, COLD_TOP, STALE)], cold_script)
    return o, m.read()


def check_cold(run):
    o, (hdr, rec) = run
    inside_bounds(o)
    assert (hdr["subjects"] == COLD_N).all()
    assert hdr["unknown_sum"].max() > 0 and hdr["unknown_sum"][-1] == 0, "`unknown` was to occur and to fall to 0"
    listed = hdr["listed"] & 0xFFFFFFFF
    assert listed[-1] < COLD_TOP and listed.max() > listed[-1]
    assert not rec[-1][int(listed[-1]):].view(np.uint64).any()        # zero-filled records


# ---- slots come and go (tests/test_census_gpu.py's scenario of that name) ----
SLOTS_TICKS = 170
SLOTS_KW = dict(fanout=4, view_slots=16, event_ring=64, query_ring=64, probe_interval=5, loss=0.01, push_pull_interval=150,
                join_sync=True, recycle_interval=20, flags=KRANDOM)


def slots_script(sim, step):
    sim.inject(5, _ffi.OP_CRASH, 300)
    sim.inject(40, _ffi.OP_REVIVE, 300)
    sim.inject(12, _ffi.OP_LEAVE, 100)
    sim.inject(50, _ffi.OP_CRASH, 2000)
    sim.inject(90, _ffi.OP_CRASH, 7)
    step(SLOTS_TICKS)


@functools.lru_cache(maxsize=None)
def slots_oracle():
    o = _ffi.Sim(load_oracle(), _ffi.make_config(N, **SLOTS_KW))
    holes = []

    def look():                                                       # is a free slot below an allocated one?
        used = np.sort(o.dump(_ffi.ARR_SLOTMAP).astype(np.int64))
        used = used[used != 0xFFFFFFFF]
        holes.append(len(used) > 0 and used.tolist() != list(range(len(used))))
    m = RollModel(o, look)
    m.start(0, 1, SLOTS_TICKS, TOP_K, STALE)
    slots_script(o, m.step)
    return o, m.read(), holes


def check_slots(run):
    o, (hdr, rec), holes = run
    cs = inside_bounds(o)
    d = np.diff(hdr["subjects"].astype(np.int64))
    assert cs["slots_recycled"] > 0 and (d > 0).any() and (d < 0).any(), "the allocated set was to grow and to shrink"
    assert any(holes), "no sample with a free slot below an allocated one"
    assert hdr["stale_max"].max() > 0


# ---- more than one chunk of slots ----
# roll_count_kernel looks at the slots in chunks of ROLL_CHUNK, a lane each, and reuses its LDS lists from one chunk to the next
# (serf_amd/csrc/serf_sim_roll.inc: #define ROLL_CHUNK 256u; tests/test_roll_gpu.py holds the source to it)
ROLL_CHUNK = 256
# dense: every node a subject, slot == id — two whole chunks and one of 88 slots
DENSE_N, DENSE_TICKS, DENSE_PERIOD = 2 * ROLL_CHUNK + 88, 60, 3
DENSE_KW = dict(fanout=3, probe_interval=5, loss=0.02, event_ring=64, query_ring=64)


def dense_script(sim, step):
    sim.inject(4, _ffi.OP_CRASH, 100)
    sim.inject(9, _ffi.OP_CRASH, DENSE_N - 3)                         # a subject of the last chunk
    sim.inject(12, _ffi.OP_LEAVE, 300)                                # one of the second
    sim.inject(30, _ffi.OP_REVIVE, 100)
    step(DENSE_TICKS)


@functools.lru_cache(maxsize=None)
def dense_oracle():
    o = _ffi.Sim(load_oracle(), _ffi.make_config(DENSE_N, **DENSE_KW))
    (m,), _ = models_run(o, [(0, DENSE_PERIOD, 100, TOP_K, STALE)], dense_script)
    return o, m.read()


def check_dense(run):
    o, (hdr, rec) = run
    inside_bounds(o)
    assert (hdr["subjects"] == DENSE_N).all() and DENSE_N > 2 * ROLL_CHUNK and DENSE_N % ROLL_CHUNK
    assert hdr["stale_max"].max() > 0 and hdr["holders_stale_alive"].max() > 0 and hdr["lag_max"].max() > 0


# sparse: 320 view slots at 1 024 nodes, a member leaves every second tick: the subjects grow one by one through the first chunk
# into the second, whose list is 1, 2, ... 35 slots long while the first stays full (a leave a tick overflows queues: not used)
GROW_N, GROW_TICKS, GROW_PERIOD, GROW_LEAVERS = 1024, 600, 10, 290
GROW_KW = dict(fanout=4, view_slots=320, event_ring=64, query_ring=64, probe_interval=5, loss=0.0, push_pull_interval=150,
               join_sync=True, recycle_interval=20, ring_overflow=4, flags=KRANDOM)


def grow_script(sim, step):
    ids = np.random.default_rng(9).choice(GROW_N, GROW_LEAVERS + 1, replace=False).tolist()
    for i, x in enumerate(ids[:GROW_LEAVERS]):
        sim.inject(2 + 2 * i, _ffi.OP_LEAVE, x)
    sim.inject(575, _ffi.OP_CRASH, ids[-1])
    sim.inject(579, _ffi.OP_REVIVE, ids[-1])
    step(GROW_TICKS)


@functools.lru_cache(maxsize=None)
def grow_oracle():
    o = _ffi.Sim(load_oracle(), _ffi.make_config(GROW_N, **GROW_KW))
    (m,), _ = models_run(o, [(0, GROW_PERIOD, 100, TOP_K, STALE)], grow_script)
    return o, m.read()


def check_grow(run):
    o, (hdr, rec) = run
    inside_bounds(o)
    sub = hdr["subjects"].astype(np.int64)
    assert sub.min() < ROLL_CHUNK < sub.max() and sub.max() % ROLL_CHUNK, "the subjects were to grow from one chunk into a second, partial one"
    assert (sub > ROLL_CHUNK).sum() >= 5 and len(set(sub[sub > ROLL_CHUNK].tolist())) >= 3       # second lists of several lengths
    assert hdr["stale_max"].max() > 0 and (hdr["stale_max"][sub > ROLL_CHUNK] > 0).any()


# ---- the interface ----
def roll_declared():
    src = re.sub(r"/\*.*?\*/", "", open(ROLL_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|uint32_t|const char\s*\*)\s*(sim_[a-z_0-9]+)\s*\(", src)))


def test_roll_header_declares_what_the_binding_binds():
    assert roll_declared() == sorted("sim_" + s for s in _ffi.ROLL_SYMBOLS)
    assert len(_ffi.ROLL_SYMBOLS) == 6


def test_hip_library_exports_the_roll():
    lib = serf_amd.load()
    dll = C.CDLL(lib.path)
    for sym in roll_declared():
        assert hasattr(dll, sym), f"{sym} missing from {lib.path}"
    fn = dll.sim_roll_version
    fn.restype = C.c_uint32
    assert fn() == 1
    assert lib.has_roll and lib.roll_version() == 1


def test_the_abi_and_the_three_older_extensions_are_what_they_were(oracle):
    """The roll is an extension: serf_sim.h, the three older headers, their symbol lists and the ABI version do not know it;
    the oracle has none."""
    assert tuple(_ffi.ABI_SYMBOLS) == ABI_SYMBOLS_15
    assert tuple(_ffi.TRACK_SYMBOLS) == TRACK_SYMBOLS_1
    assert tuple(_ffi.SERIES_SYMBOLS) == SERIES_SYMBOLS_1
    assert tuple(_ffi.CENSUS_SYMBOLS) == CENSUS_SYMBOLS_1
    assert test_abi.declared_symbols() == sorted("sim_" + s for s in ABI_SYMBOLS_15)
    older = set(_ffi.ABI_SYMBOLS) | set(_ffi.TRACK_SYMBOLS) | set(_ffi.SERIES_SYMBOLS) | set(_ffi.CENSUS_SYMBOLS)
    assert not set(_ffi.ROLL_SYMBOLS) & older
    lib = serf_amd.load()
    assert lib.abi_version() == 15 and oracle.abi_version() == 15
    assert lib.track_version() == 1 and lib.series_version() == 1 and lib.census_version() == 1
    assert not oracle.has_roll and oracle.roll_version() is None
    odll = C.CDLL(oracle.path)
    for s in _ffi.ROLL_SYMBOLS:
        assert not hasattr(odll, "osim_" + s)
    o = _ffi.Sim(oracle, _ffi.make_config(64))
    for call in (o.roll_start, o.roll_count, o.roll_read, o.roll_stop, o.roll_now):
        with pytest.raises(NotImplementedError):
            call()


def test_roll_struct_layout_matches_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "serf_sim_roll.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %u %u %u %u %u %u %u\\n",sizeof(sim_roll_node),sizeof(sim_roll_header),'
                    "offsetof(sim_roll_node,w[6]),offsetof(sim_roll_header,w[16]),SIM_ROLL_TOP_MAX,SIM_ROLL_MAX_SAMPLES,"
                    "SIM_ROLL_VERSION,SIM_ROLL_BY_STALE,SIM_ROLL_BY_ACCUSED,SIM_ROLL_BY_MISSED,SIM_ROLL_HEADER_WORDS);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(prog)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [_ffi.ROLL_NODE_DTYPE.itemsize, _ffi.ROLL_HEADER_DTYPE.itemsize, 48, 128, _ffi.ROLL_TOP_MAX, _ffi.ROLL_MAX_SAMPLES,
                   1, STALE, ACCUSED, MISSED, _ffi.ROLL_HEADER_WORDS]
    assert got[:2] == [64, 256] and got[4] == 64
    # the records' fields are the tables' words, in order
    off = {n: _ffi.ROLL_NODE_DTYPE.fields[n][1] // 8 for n in _ffi.ROLL_NODE_DTYPE.names}
    assert off == dict(id=0, stale=1, unknown=2, false_failed=3, suspects=4, stale_alive=5, lag=6, behind=7)
    off = {n: _ffi.ROLL_HEADER_DTYPE.fields[n][1] // 8 for n in _ffi.ROLL_HEADER_DTYPE.names}
    assert off == dict(tick=0, running=1, subjects=2, listed=3, current=4, stale_sum=5, stale_max=6, unknown_sum=7, accusers_failed=8,
                       false_failed_sum=9, accusers_suspect=10, suspects_sum=11, holders_stale_alive=12, stale_alive_sum=13,
                       lag_sum=14, lag_max=15, stale_bins=16)
    h, r = _ffi.roll_split(np.arange(2 * (32 + 8 * 3), dtype=np.uint64), 3)
    assert h.shape == (2,) and r.shape == (2, 3) and int(h["tick"][1]) == 56 and int(r["id"][1, 2]) == 56 + 32 + 16


def test_stale_bins():
    assert [stale_bin(x) for x in (0, 1, 2, 3, 4, 7, 8, 16383, 16384, 32767, 32768, 1 << 20)] == [0, 1, 2, 2, 3, 3, 4, 14, 15, 15, 15, 15]


def test_sampling_rule_of_the_model(oracle):
    o = _ffi.Sim(oracle, _ffi.make_config(256, fanout=3))
    m = RollModel(o)
    m.step(4)
    m.start(first_tick=10, period=7, capacity=3, top_k=5, rank_by=ACCUSED)
    m.step(40)
    assert m.count() == (3, 2)                                   # ticks 10, 17, 24 taken; 31, 38 dropped
    hdr, rec = m.read()
    assert hdr["tick"].tolist() == [11, 18, 25] and rec.shape == (3, 5)
    assert (hdr["subjects"] == 256).all() and (hdr["running"] == 256).all() and (hdr["current"] == 256).all()
    assert (hdr["listed"] == ACCUSED << 32).all() and not rec.view(np.uint64).any()      # nobody to list: all agree
    assert (hdr["stale_bins"][:, 0] == 256).all() and not hdr["stale_bins"][:, 1:].any()
    m.stop()
    m.start(first_tick=0, period=2, capacity=100)               # a first tick that has passed: now (44)
    m.step(5)
    assert m.count() == (3, 0) and m.read()[0]["tick"].tolist() == [45, 47, 49]
    h, t, every = m.now(3, MISSED, nodes=True)
    assert int(h["tick"]) == 49 and len(t) == 3 and len(every) == 256 and int(h["listed"]) == MISSED << 32
    assert every["id"].tolist() == [i | 1 << 32 for i in range(256)]


def test_model_equals_members_and_the_census_model_at_256_nodes(oracle):
    """Two independent routes on the oracle.  sim_members(observer) for every running observer rebuilds `unknown`, `false_failed`
    and `stale_alive` of every node — the counts `st` and `known` alone define (sim_members shows neither the memberlist state
    nor the incarnation) — and `behind` as far as Lamport times decide it, a lower bound.  The census model's header words 6, 8
    and 10 are the roll's 9, 11 and 13 — which covers `suspects`."""
    n = 256
    o = _ffi.Sim(oracle, _ffi.make_config(n, fanout=3, view_slots=32, probe_interval=5, loss=0.02, push_pull_interval=150,
                                          join_sync=True, event_ring=64, query_ring=64))
    for t, c in ((3, 17), (6, 200), (9, 90)):
        o.inject(t, _ffi.OP_CRASH, c)
    o.inject(81, _ffi.OP_REVIVE, 17)                               # (one tick before a look: it runs, and is still held Failed)
    seen = dict(false_failed=0, suspects=0, stale_alive=0, behind=0, lag=0)
    for stretch, act in ((12, lambda: o.leave(5)), (30, lambda: None), (40, lambda: o.join(5, 7)), (30, lambda: None)):
        o.step(stretch)
        act()
        for by in (STALE, ACCUSED, MISSED):
            hdr, rec = split(sample(o, 16, by), 16)
            hdr, rec = hdr[0], rec[0]
            w, up, ns = node_records(o)
            every = np.ascontiguousarray(w).view(_ffi.ROLL_NODE_DTYPE).reshape(-1)
            rows = o.dump(_ffi.ARR_ROWS)
            run = (rows["flags"] & 1) != 0
            assert up.tolist() == run.tolist() and int(hdr["running"]) == int(run.sum())
            slot_of = o.dump(_ffi.ARR_SLOTMAP)
            subj = np.nonzero(slot_of != 0xFFFFFFFF)[0]
            assert int(hdr["subjects"]) == len(subj) == ns and ns >= 4
            st_all, lt_all = zip(*(o.members(int(obs)) for obs in np.nonzero(run)[0]))
            st, lt = np.array(st_all)[:, subj].astype(np.int64), np.array(lt_all)[:, subj]       # [observer][subject]
            known = st != _ffi.STATUS_NONE
            anyknown, ltmax = known.any(axis=0), np.where(known, lt, 0).max(axis=0)
            obs = every[run]
            assert obs["unknown"].tolist() == (~known & anyknown).sum(axis=1).tolist()
            assert obs["false_failed"].tolist() == (run[subj] & (st == _ffi.STATUS_FAILED)).sum(axis=1).tolist()
            assert obs["stale_alive"].tolist() == (~run[subj] & (st == _ffi.STATUS_ALIVE)).sum(axis=1).tolist()
            assert (obs["behind"] >= (known & (lt < ltmax)).sum(axis=1)).all()
            assert obs["lag"].tolist() == np.where(known, ltmax - np.where(known, lt, ltmax), 0).sum(axis=1).tolist()
            assert (obs["stale"] == obs["unknown"] + obs["behind"]).all()
            assert not every[~run].view(np.uint64).reshape(-1, 8)[:, 1:].any() and (every["id"] >> 32).tolist() == run.astype(int).tolist()
            # the header from the records
            assert int(hdr["stale_sum"]) == int(obs["stale"].sum()) and int(hdr["stale_max"]) == int(obs["stale"].max())
            assert int(hdr["current"]) == int((obs["stale"] == 0).sum()) == int(hdr["stale_bins"][0])
            assert int(hdr["stale_bins"].sum()) == int(run.sum())
            assert int(hdr["lag_sum"]) == int(obs["lag"].sum()) and int(hdr["lag_max"]) == int(obs["lag"].max())
            # the census model: pairs counted per subject there, per observer here
            ch = census_sample(o, 32)[:16]
            assert (int(hdr["false_failed_sum"]), int(hdr["suspects_sum"]), int(hdr["stale_alive_sum"])) == (int(ch[6]), int(ch[8]), int(ch[10]))
            assert int(hdr["suspects_sum"]) == int(obs["suspects"].sum())
            # the listed ones: descending score, ties in ascending id, nobody with score 0, nobody better left out
            score = score_of(w, by)
            listed = int(hdr["listed"]) & 0xFFFFFFFF
            assert int(hdr["listed"]) >> 32 == by and listed == min(16, int((score > 0).sum()))
            ids = (rec["id"][:listed] & 0xFFFFFFFF).astype(np.int64)
            keys = [(-int(score[i]), int(i)) for i in ids]
            assert keys == sorted(keys) and len(set(ids.tolist())) == listed
            assert rec[:listed].tolist() == every[ids].tolist() and not rec[listed:].view(np.uint64).any()
            rest = np.setdiff1d(np.arange(n), ids)
            if listed:
                assert listed < 16 or (-int(score[rest].max()), int(rest[np.argmax(score[rest])])) > keys[-1]
            for k in seen:
                seen[k] += int(obs[k].sum())
    assert all(v > 0 for v in seen.values()), seen
    inside_bounds(o)


@pytest.mark.parametrize("variant", VARIANTS)
def test_census_scenarios_are_nontrivial_on_the_oracle(variant):
    check_census_scenario(variant, census_oracle(variant))


def test_busy_is_nontrivial_on_the_oracle():
    check_busy(busy_oracle())


def test_cold_join_is_nontrivial_on_the_oracle():
    check_cold(cold_oracle())


def test_slots_come_and_go_on_the_oracle():
    check_slots(slots_oracle())


def test_more_than_one_chunk_of_slots_on_the_oracle():
    check_dense(dense_oracle())
    check_grow(grow_oracle())
