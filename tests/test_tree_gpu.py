"""The rumour tree of the HIP library (include/serf_sim_tree.h) against the reference model (tests/tree_model.py) on the oracle,
run side by side with it: behind every step every word of every sample, all three planes and the children through tree_links,
tree_summary, tree_top and tree_path of a few nodes are compared exactly; at the end the digest is compared with the oracle's.
The scenarios are those of tests/test_tree.py; the shapes are the observer shapes of tests/test_observer_shapes.py — ragged,
tiny, idle, and one size beyond what one pass of the capped grid covers (tree_latch_kernel, tree_carry_kernel and
tree_cand_kernel have the series' pass loop and grid cap).  Then the sampling rules, the errors and their order, a tree across
sim_restore, a tree beside every other observer, and neutrality.  Every call goes through Sim.tree_*: a library without the
symbols fails these tests, it does not skip them."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from serf_amd.workload import apply_schedule
from tests import test_observer_shapes as shapes
from tests import test_traffic as tt
from tests import test_tree as tr
from tests.test_traffic_gpu import same_records, words
from tests.traffic_model import k_random_nodes_all
from tests.tree_model import TreeModel

pytestmark = pytest.mark.gpu
NONE = _ffi.TREE_NONE


def path_nodes(m, e):
    """A few nodes whose chains are worth chasing: the deepest, the latest, the first and the last node, one without an arrival."""
    n = m.arrival.shape[1]
    pick = {0, n - 1, int(np.argmax(m.hop[e])), int(np.argmax(m.arrival[e]))}
    none = np.nonzero(m.arrival[e] == 0)[0]
    return sorted(pick | ({int(none[0])} if len(none) else set()))


def same_reads(g, m, what, top_ks=(10,), entries=None):
    """The samples, and of every entry (or of `entries`): all links, a slice of them, the ranking, a few paths; the summary."""
    n, ne = int(g.cfg.n_nodes), len(m.entries)
    assert g.tree_count() == m.count(), what
    got, want = g.tree_read(), m.read()
    same_records(got[0], want[0], f"{what}: headers")
    same_records(got[1], want[1], f"{what}: entries")
    same_records(g.tree_summary(), m.summary(), f"{what}: summary")
    for e in range(ne) if entries is None else entries:
        same_records(g.tree_links(e), m.links(e), f"{what}: links of entry {e}")
        if n > 5:
            same_records(g.tree_links(e, 2, 3), m.links(e, 2, 3), f"{what}: links 2 .. 4 of entry {e}")
            assert len(g.tree_links(e, n, 0)) == 0
        for k in top_ks:
            same_records(g.tree_top(e, k), m.top(e, k), f"{what}: top {k} of entry {e}")
        for node in path_nodes(m, e):
            gi, gt = g.tree_path(e, node)
            mi, mt = m.path(e, node)
            assert gt == mt and gi.tolist() == mi.tolist(), f"{what}: path of node {node}, entry {e}"
            gi, gt = g.tree_path(e, node, 2)
            assert gt == mt and gi.tolist() == mi[:2].tolist()


def pair(n, kw, ops):
    """A fresh oracle with its model and a fresh HIP handle, the schedule injected into both."""
    o = tt.make(n, kw)
    g = serf_amd.create(n, **kw)
    apply_schedule(o, ops)
    apply_schedule(g, ops)
    return o, TreeModel(o), g


def side_by_side(n, kw, ops, entries, ticks, what, chunk=1, check=None, inject=None, sparse=False, bounded=True, **start):
    """Both sides started alike and stepped `chunk` ticks at a time, everything compared behind every step (sparse: the samples
    and entry 0 behind every step, everything at the end); at the end the rankings of 1 and 64 as well, the digest, and
    check(o, m) — that the scenario moved what it is for."""
    o, m, g = pair(n, kw, ops)
    start = dict(dict(first_tick=0, capacity=ticks), **start)
    m.start(entries, **start)
    g.tree_start(entries, **start)
    if inject:
        inject(o), inject(g)
    for t in range(0, ticks, chunk):
        m.step(min(chunk, ticks - t))
        g.step(min(chunk, ticks - t))
        same_reads(g, m, f"{what}, tick {o.tick}", entries=(0,) if sparse else None)
    same_reads(g, m, f"{what}, the end", top_ks=(1, 10, 64))
    assert g.digest() == o.digest(), what
    cs = o.cluster_stats()
    assert not bounded or (cs["overflow"] == 0 and cs["ops_dropped"] == 0), "the run stays inside the model's bounds"
    if check:
        check(o, m)
    g.close()
    o.close()


def moved(n):
    def check(o, m):
        s = m.summary()
        assert s["reached"][-1] == 0, "the entry that is never injected"
        if n > 1:
            assert s["reached"][:-1].sum() > 0
        if n >= 63:
            assert (s["reached"] - s["orphans"]).sum() > n and s["depth"].max() >= 2 and s["most_children"].max() >= 2
            assert m.read()[1]["fresh"].sum() > 0 and m.read()[1]["copies"].sum() > m.read()[1]["fresh"].sum()
    return check


# ---- 1. shapes ----
@pytest.mark.parametrize("fan", sorted(tr.FANOUTS))
@pytest.mark.parametrize("n", shapes.RAGGED_SIZES)
def test_ragged_sizes(hiplib, n, fan):
    """20 ticks of the churn schedule with a rejoin: user events, one JOIN, one LEAVE, one QUERY entry where the run has them, and
    one entry that is never injected.  At 1, 2 and 3 nodes there are fewer other nodes than the fan-out."""
    entries = tr.churn_entries(n, fan)
    if n >= 63:
        kinds = [e[0] for e in entries]
        assert _ffi.K_JOIN in kinds and _ffi.K_LEAVE in kinds and _ffi.K_EVENT in kinds
    side_by_side(n, tt.churn_kw(n, fan), tr.tree_ops(n), entries, tt.CHURN_TICKS, f"ragged({n}) {fan}", check=moved(n), sparse=n >= 1000)


@pytest.mark.parametrize("fan", sorted(tr.FANOUTS))
def test_64_entries_257_nodes(hiplib, fan):
    """Every bit of the masks: 63 user events from 63 nodes, seven a tick, and the entry that is never injected."""
    n, ticks = 257, 16
    kw = tr.quiet_kw(n, fan, retransmit_mult=2, ring_overflow=16)      # (seven keys at one Lamport time: a bucket and an overflow row)
    ops = tr.many_ops(n)
    entries = tr.dry_entries(n, tuple(sorted(kw.items())), tuple(ops), ticks, events=63)

    def check(o, m):
        s = m.summary()
        assert len(m.entries) == 64 and (s["reached"][:-1] > n // 2).all() and (s["orphans"][:-1] == 1).all() and s["reached"][-1] == 0
    side_by_side(n, kw, ops, entries, ticks, f"64 entries {fan}", check=check, sparse=True)


@pytest.mark.parametrize("fan", sorted(tr.FANOUTS))
def test_multi_page_packets_257_nodes(hiplib, fan):
    """pkt_records = 16 with the burst: carriers on pages 2 - 4, and packets mapped to several slots."""
    entries = tr.churn_entries(257, fan, burst=tt.PKT16_BURST, more=tuple(sorted(tt.PKT16.items())))

    def check(o, m):
        assert m.read()[1]["copies"].sum() > 0 and m.summary()["reached"].sum() > 257
    side_by_side(257, tt.churn_kw(257, fan, **tt.PKT16), tr.tree_ops(257, burst=tt.PKT16_BURST), entries, tt.CHURN_TICKS, f"pkt16 {fan}",
                 check=check, sparse=True)


@pytest.mark.parametrize("fan", sorted(tr.FANOUTS))
def test_loss_257_nodes(hiplib, fan):
    n, _, more, origins, ticks = tr.QUIET["257_loss"]
    kw = tr.quiet_kw(n, fan, **more)
    entries = tr.inject_events(tt.make(n, kw), origins)

    def check(o, m):
        assert m.summary()["orphans"].tolist() == [1, 1, 1] and m.summary()["depth"].min() >= 4
    side_by_side(n, kw, [], entries, ticks, f"loss {fan}", check=check, inject=lambda s: tr.inject_events(s, origins))


@pytest.mark.parametrize("fan", sorted(tr.FANOUTS))
def test_swim_and_push_pull_1000_nodes(hiplib, fan):
    kw = tt.churn_kw(tr.SWIM_N, fan, **tr.SWIM_KW)
    origins = (5, 400, 900)
    entries = tr.inject_events(tt.make(tr.SWIM_N, kw), origins)

    def check(o, m):
        assert (m.summary()["orphans"] > 1).all(), "push-pull delivers without a packet"
    side_by_side(tr.SWIM_N, kw, [], entries, tr.SWIM_TICKS, f"swim {fan}", check=check, sparse=True, bounded=False,
                 inject=lambda s: tr.inject_events(s, origins))       # (32 view slots at 1 000 nodes: suspicions about members without a slot are dropped, on both sides alike)


def test_vshards_2048_nodes_bijection(hiplib):
    """vshards = 4 on one handle that holds every node: the bijection's inverse across virtual shards."""
    entries = tr.churn_entries(2048, "bijection", more=(("vshards", 4),))
    side_by_side(2048, tt.churn_kw(2048, "bijection", vshards=4), tr.tree_ops(2048), entries, tt.CHURN_TICKS, "vshards 4", check=moved(2048),
                 sparse=True)


@pytest.mark.parametrize("fan", sorted(tr.FANOUTS))
@pytest.mark.parametrize("n", shapes.IDLE_SIZES)
def test_nobody_runs(hiplib, n, fan):
    """Every node crashes at tick 5: behind that nothing is latched and nothing is in flight."""
    ops = [(shapes.IDLE_CRASH, _ffi.OP_CRASH, x, 0, 0) for x in range(n)]
    kw = tt.churn_kw(n, fan)
    entries = tr.inject_events(tt.make(n, kw), (0,)) + [tr.NEVER]

    def check(o, m):
        hdr, rec = m.read()
        assert hdr["running"].tolist() == [n] * shapes.IDLE_CRASH + [0] * (shapes.IDLE_TICKS - shapes.IDLE_CRASH)
        late = words(hdr[shapes.IDLE_CRASH + 1:]).reshape(-1, _ffi.TREE_HEADER_WORDS)
        assert not late[:, 3:].any() and rec["reached"][-1][0] >= 1
    side_by_side(n, kw, ops, entries, shapes.IDLE_TICKS, f"nobody_runs({n}) {fan}", check=check, inject=lambda s: tr.inject_events(s, (0,)))


SECOND_N, SECOND_TICKS = tr.TREE_GRID * shapes.BLOCK + shapes.SECOND_PASS, 4


def test_second_pass(hiplib):
    """TREE_GRID * BLOCK + 65 nodes: the pass loops of the latch, carry and candidate kernels take a second turn, of one whole wave
    and one lane.  One event's origin lies in that pass — its children in the first —, the other's origin is a node of the first
    pass that draws a node of the second at tick 0: links across the passes both ways.  Compared behind the last tick."""
    n, first = SECOND_N, tr.TREE_GRID * shapes.BLOCK
    tr.test_the_cap_is_the_sources()
    assert n == shapes.SERIES_N == 262209
    kw = dict(shapes.BIG_KW)
    tg = k_random_nodes_all(int(_ffi.make_config(n, **kw).seed), 0, n, int(kw["fanout"]))
    hits = np.nonzero((tg >= first).any(axis=1))[0]
    origins = (n - 3, int(hits[hits < first][0]))
    entries = tr.inject_events(tt.make(n, kw), origins)

    def check(o, m):
        up, down = m.links(0), m.links(1)
        assert up["arrival"][origins[0]] == 1 and up["children"][origins[0]] >= 2 and (up["parent"][:first] >= first).sum() >= 2
        assert ((down["arrival"][first:] != 0) & (down["parent"][first:] < first)).any(), "a child in the second pass of a parent in the first"
        assert m.summary()["depth"].min() >= 2
    side_by_side(n, kw, [(2, _ffi.OP_CRASH, n - 1, 0, 0)], entries, SECOND_TICKS, "second pass", chunk=SECOND_TICKS, check=check,
                 inject=lambda s: tr.inject_events(s, origins))


# ---- 2. sampling ----
def test_a_later_start_a_full_buffer_and_a_restart(hiplib):
    """Started behind tick 3 with the event travelling: every holder an orphan.  Room for 2 samples; what is due behind that is
    counted and latches nothing.  Then stop and start again: the planes are zero again."""
    n, kw = 257, tr.quiet_kw(257, "krandomnodes")
    o, m, g = pair(n, kw, [])
    entries = tr.inject_events(o, (5,))
    assert tr.inject_events(g, (5,)) == entries
    o.step(3)
    g.step(3)
    m.start(entries, 1, 2)
    g.tree_start(entries, 1, 2)
    m.step(1)
    g.step(1)
    same_reads(g, m, "a later start, the first sample")
    hdr, rec = g.tree_read()
    assert hdr["tick"].tolist() == [4] and rec["new_orphans"][0][0] == rec["reached"][0][0] > 4
    m.step(6)
    g.step(6)                                                              # ONE call
    assert g.tree_count() == m.count() == (2, 5) and g.tree_read()[0]["tick"].tolist() == [4, 5]
    same_reads(g, m, "a later start, a full buffer", top_ks=(1, 10, 64))
    assert g.tree_summary()["reached"][0] == g.tree_read()[1]["reached"][-1][0] < n
    m.stop()
    g.tree_stop()
    assert g.tree_count() == (0, 0)
    m.start(entries, 0, 8)
    g.tree_start(entries, 0, 8)
    assert not g.tree_links(0)["arrival"].any() and g.tree_summary()["reached"][0] == 0
    m.step(3)
    g.step(3)
    same_reads(g, m, "started again", top_ks=(1, 10, 64))
    assert g.tree_summary()["orphans"][0] == g.tree_summary()["reached"][0] == n, "everybody held it at the first sample"
    assert g.digest() == o.digest()
    g.close()
    o.close()


def test_one_step_call_against_single_steps_with_reads_between(hiplib):
    """sim_step(h, 20) against twenty sim_step(h, 1) with every read between them: a read changes nothing."""
    n, kw = 1000, tt.churn_kw(1000, "bijection")
    entries = tr.churn_entries(n, "bijection")
    a, b = serf_amd.create(n, **kw), serf_amd.create(n, **kw)
    for s in (a, b):
        apply_schedule(s, tr.tree_ops(n))
        s.tree_start(entries, 0, tt.CHURN_TICKS)
    a.step(tt.CHURN_TICKS)
    for _ in range(tt.CHURN_TICKS):
        b.step(1)
        b.tree_links(0, 1, 5), b.tree_top(1, 3), b.tree_summary(), b.tree_read(0, 1), b.tree_path(0, 7)
    for x, y in zip(a.tree_read(), b.tree_read()):
        same_records(x, y, "step(20) against 20 step(1)")
    for e in range(len(entries)):
        same_records(a.tree_links(e), b.tree_links(e), "step(20) against 20 step(1): the links")
    a.close()
    b.close()


# ---- 3. neutrality, and the other observers ----
@pytest.mark.parametrize("fan", sorted(tr.FANOUTS))
def test_digests_with_and_without_the_tree(hiplib, fan):
    n, ticks, kw = 1000, 40, tt.churn_kw(1000, fan, probe_interval=5, loss=0.01)
    ops = tr.tree_ops(n, ticks)
    entries = tr.churn_entries(n, fan)
    o = tt.make(n, kw)
    with_tree, without = serf_amd.create(n, **kw), serf_amd.create(n, **kw)
    for s in (o, with_tree, without):
        apply_schedule(s, ops)
    with_tree.tree_start(entries, 0, ticks)
    for s in (o, with_tree, without):
        s.step(ticks)
    assert with_tree.tree_count() == (ticks, 0) and with_tree.tree_read()[1]["copies"].sum() > 0
    assert with_tree.digest() == without.digest() == o.digest()
    assert with_tree.snapshot().tobytes() == without.snapshot().tobytes(), "an image holds no tree"
    assert without.tree_count() == (0, 0)
    for s in (o, with_tree, without):
        s.close()


def test_beside_every_other_observer(hiplib):
    """The tree with the series, the census, the roll, the ledger, the detection log, the spread map, the traffic meter and a
    tracker running on the same handle: its words are the model's, its arrivals the spread map's, its copies the ledger's."""
    n, fan, ticks = 1000, "krandomnodes", tt.CHURN_TICKS
    kw = tt.churn_kw(n, fan, probe_interval=5)
    entries = list(tr.churn_entries(n, fan, more=(("probe_interval", 5),)))
    o, m, g = pair(n, kw, tr.tree_ops(n))
    m.start(entries, 0, ticks)
    g.series_start(0, 1, ticks), g.census_start(0, 1, ticks, 8), g.roll_start(0, 1, ticks), g.ledger_start(entries, 0, 1, ticks)
    g.detect_start(0, 1, ticks), g.spread_start(entries, 0, 1, ticks), g.traffic_start(0, 1, ticks)
    ids = g.track_add([_ffi.rumour_tracker(*entries[0])])
    g.tree_start(entries, 0, ticks)
    m.step(ticks)
    g.step(ticks)
    same_reads(g, m, "beside the other observers")
    hdr, rec = g.tree_read()
    assert rec["copies"].tolist() == g.ledger_read()[1]["in_flight"].tolist() and rec["copies"].sum() > 0
    for e in range(len(entries)):
        assert g.tree_links(e)["arrival"].tolist() == g.spread_map(e).tolist()
    assert g.traffic_count() == g.series_count() == (ticks, 0) and len(g.track_read(ids)) == 1
    assert g.digest() == o.digest()
    g.close()
    o.close()


# ---- 4. errors and states ----
def test_errors_leave_everything_as_it_was(hiplib):
    n, kw = 257, tr.quiet_kw(257, "krandomnodes")
    ok = [(_ffi.K_EVENT, 0x7700, 1), (_ffi.K_JOIN, 3, 1), (_ffi.K_QUERY, 9, 2)]
    every = lambda s: (lambda: s.tree_start(ok, 0, 8), s.tree_count, lambda: s.tree_read(0, 0), s.tree_stop, lambda: s.tree_links(0, 0, 1),
                       s.tree_summary, lambda: s.tree_path(0, 0), lambda: s.tree_top(0, 3))
    sh = serf_amd.create(n, force_sharded=True, **kw)                     # a shard has no tree
    for call in every(sh):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    o, m, g = pair(n, kw, [])
    assert g.tree_count() == (0, 0)
    for call in every(g)[2:]:                                              # no tree yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    bad = ([], [(0, 1, 1)], [(_ffi.K_ALIVE, 1, 1)], [(_ffi.K_EVENT, 0, 1)], [(_ffi.K_JOIN, n, 1)], [(_ffi.K_EVENT, 5, 1 << 48)],
           [ok[0], ok[1], ok[0]], [(_ffi.K_EVENT, 1 + i, 1) for i in range(65)])
    for es in bad:
        with pytest.raises(_ffi.SimError) as ei:
            g.tree_start(es, 0, 8)
        assert ei.value.code == _ffi.EINVAL and g.tree_count() == (0, 0), es
    for args in ((0, 0), (0, _ffi.TREE_MAX_SAMPLES + 1)):
        with pytest.raises(_ffi.SimError) as ei:
            g.tree_start(ok, *args)
        assert ei.value.code == _ffi.EINVAL and g.tree_count() == (0, 0)
    f, u, ref = g.lib.f, _ffi.C.c_uint32, _ffi.C.byref
    assert f["tree_start"](g.h, None, 3, 0, 8) == _ffi.EINVAL and f["tree_start"](None, _ffi.spread_entries(ok), 3, 0, 8) == _ffi.EINVAL
    # arguments that can be judged without a tree are SIM_EINVAL before "no tree" is SIM_ESTATE
    buf = np.zeros(4096, np.uint64)
    a, b = u(77), u(78)

    def bad_arguments():
        assert f["tree_links"](g.h, 0, 0, 1, None) == _ffi.EINVAL
        for first, cnt in ((n, 1), (0, n + 1), (n - 1, 2), (0xFFFFFFFF, 2)):
            assert f["tree_links"](g.h, 0, first, cnt, buf.ctypes.data) == _ffi.EINVAL
        assert f["tree_summary"](g.h, None) == _ffi.EINVAL
        for top_k in (0, 65):
            assert f["tree_top"](g.h, 0, top_k, buf.ctypes.data) == _ffi.EINVAL
        assert f["tree_top"](g.h, 0, 8, None) == _ffi.EINVAL
        assert f["tree_path"](g.h, 0, 0, None, 4, ref(a), ref(b)) == _ffi.EINVAL
        assert f["tree_path"](g.h, 0, 0, buf.ctypes.data, 4, None, ref(b)) == _ffi.EINVAL
        assert f["tree_path"](g.h, 0, 0, buf.ctypes.data, 4, ref(a), None) == _ffi.EINVAL
        assert f["tree_path"](g.h, 0, n, buf.ctypes.data, 4, ref(a), ref(b)) == _ffi.EINVAL
        assert f["tree_count"](g.h, None, ref(b)) == _ffi.EINVAL and f["tree_count"](g.h, ref(a), None) == _ffi.EINVAL
        assert f["tree_count"](None, ref(a), ref(b)) == _ffi.EINVAL
        assert f["tree_read"](g.h, 0, 0, None, 64, ref(a)) == _ffi.EINVAL and f["tree_read"](g.h, 0, 0, buf.ctypes.data, 64, None) == _ffi.EINVAL
        assert (a.value, b.value) == (77, 78) and not buf.any()
    bad_arguments()
    assert f["tree_links"](g.h, 9, 0, 1, buf.ctypes.data) == _ffi.ESTATE, "an entry is judged against the running tree: behind `no tree`"
    entries = tr.inject_events(o, (5,)) + ok[1:]
    tr.inject_events(g, (5,))
    m.start(entries, 0, 8)
    g.tree_start(entries, 0, 8)
    m.step(3)
    g.step(3)
    same_reads(g, m, "before the errors")
    bad_arguments()                                                        # the same with a tree running
    for es in bad[:4]:                                                     # bad arguments before "already running"
        with pytest.raises(_ffi.SimError) as ei:
            g.tree_start(es, 0, 8)
        assert ei.value.code == _ffi.EINVAL
    with pytest.raises(_ffi.SimError) as ei:
        g.tree_start(ok, 0, 0)
    assert ei.value.code == _ffi.EINVAL
    with pytest.raises(_ffi.SimError) as ei:
        g.tree_start(ok, 0, 8)
    assert ei.value.code == _ffi.ESTATE
    for first, cnt in ((0, 4), (3, 1), (4, 0)):                           # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.tree_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL
    stride = _ffi.TREE_HEADER_WORDS + 3 * _ffi.TREE_ENTRY_WORDS
    small, got = np.zeros(2 * stride, np.uint64), u(77)
    assert f["tree_read"](g.h, 0, 3, small.ctypes.data, small.size, ref(got)) == _ffi.EINVAL and got.value == 77 and not small.any()
    assert f["tree_links"](g.h, 3, 0, 1, buf.ctypes.data) == _ffi.EINVAL and f["tree_top"](g.h, 3, 8, buf.ctypes.data) == _ffi.EINVAL
    assert f["tree_path"](g.h, 3, 0, buf.ctypes.data, 4, ref(a), ref(b)) == _ffi.EINVAL and (a.value, b.value) == (77, 78) and not buf.any()
    ids, total = g.tree_path(0, 5, 0)                                      # cap 0: the length alone
    assert len(ids) == 0 and total == 1
    same_reads(g, m, "after the errors")
    m.step(2)
    g.step(2)
    same_reads(g, m, "two ticks after the errors")
    g.close()
    o.close()
    t = serf_amd.create(256, fanout=3)                                   # inside a tick
    t.tree_start(ok, 0, 8)
    t.step(2)
    t.step_begin()
    for call in every(t):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                                   # a handle destroyed with a tree running
    g.tree_start(ok, 0, 4)
    g.step(6)
    assert g.tree_count() == (4, 2) and g.tree_read()[0]["tick"].tolist() == [1, 2, 3, 4]
    g.close()


# ---- 5. restore ----
RESTORE_T = 2


@pytest.mark.parametrize("fan", sorted(tr.FANOUTS))
def test_a_tree_across_a_restore(hiplib, fan):
    """sim_restore takes a fresh handle.  A tree started at tick 0 on a fresh handle that is then restored to tick 2 stays as it
    is: the first sample behind the restore finds no candidates stamped 2 and latches every holder of the image as an orphan; from
    the second sample on the packets name the parents.  Then a tree started on a handle that was restored first.  The reference:
    the model on an oracle that restores the same image."""
    n, kw = 257, tr.quiet_kw(257, fan)
    src = tt.make(n, kw)
    entries = tr.inject_events(src, (5, 77))
    src.step(RESTORE_T)
    img = src.snapshot()
    for started_first in (True, False):
        o, g = tt.make(n, kw), serf_amd.create(n, **kw)
        m = TreeModel(o)
        if started_first:
            m.start(entries, 0, 16)
            g.tree_start(entries, 0, 16)
        o.restore(img)
        g.restore(img)
        assert g.tick == o.tick == RESTORE_T and g.tree_count() == (0, 0)
        if not started_first:
            m.start(entries, 0, 16)
            g.tree_start(entries, 0, 16)
        m.step(1)
        g.step(1)
        what = f"a tree {'before' if started_first else 'behind'} a restore, {fan}"
        same_reads(g, m, what + ", the first tick")
        hdr, rec = g.tree_read()
        assert hdr["tick"].tolist() == [RESTORE_T + 1] and (rec["new"][0] == rec["new_orphans"][0]).all() and rec["new"][0].min() > 1
        for _ in range(6):
            m.step(1)
            g.step(1)
            same_reads(g, m, what)
        s = g.tree_summary()
        assert (s["orphans"] == rec["new_orphans"][0]).all() and (s["reached"] > 4 * s["orphans"]).all() and s["depth"].min() >= 2
        assert g.snapshot().tobytes() == o.snapshot().tobytes() and g.digest() == o.digest()
        g.close()
        o.close()
    src.close()
