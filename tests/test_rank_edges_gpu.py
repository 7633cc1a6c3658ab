"""The edges of the ranking in two levels (rank_candidates / rank_merge, serf_sim_observe.inc) behind its four users — traffic_top,
tree_top, spread_late, roll_now — where their copies could once have disagreed: BLOCK + 1 nodes, so that the second workgroup's
candidate list is one entry and a terminator; a ranking of 64 read before any value differs, when every key ties and only the id
orders them; three nodes for 64 places, the unused ones filled each observer's own way; and two nodes with equal scores on either
side of the workgroup boundary, which only the second word of the spread map's key tells apart.  Expected values are the reference
models' on the oracle, compared exactly.  What tests/test_*_gpu.py already assert of these (rankings of 64 at 257 and 3 nodes at the
END of their ragged runs) is listed in profiles/observer_kit.md."""
import pytest

import serf_amd
from serf_amd import _ffi
from serf_amd.workload import apply_schedule
from tests import test_observer_shapes as shapes
from tests import test_traffic as tt
from tests import test_tree as tr
from tests.roll_model import RollModel
from tests.spread_model import SpreadModel
from tests.test_roll_gpu import same_now
from tests.test_traffic_gpu import same_records, words
from tests.traffic_model import TrafficModel
from tests.tree_model import TreeModel

pytestmark = pytest.mark.gpu
N, FEW, TOP, TICKS, FAN = shapes.BLOCK + 1, 3, 64, 10, "krandomnodes"
NO_ID = 0xFFFFFFFF
ROLL_BYS = (_ffi.ROLL_BY_STALE, _ffi.ROLL_BY_ACCUSED, _ffi.ROLL_BY_MISSED)
SPREAD_BYS = (_ffi.SPREAD_BY_MISSED, _ffi.SPREAD_BY_LATE)


def no_tracker(spec):
    return 0


class Churn:
    """The small churn schedule of tests/test_traffic.py with the tree's rejoin, every operation injected up front."""
    @staticmethod
    def kw(n):
        return tt.churn_kw(n, FAN)

    @staticmethod
    def before(sim, n):
        apply_schedule(sim, tr.tree_ops(n, TICKS))

    @staticmethod
    def drive(sim, n, step):
        step(TICKS)


class Traffic(Churn):
    def __init__(self, o, g, n):
        self.m = TrafficModel(o)
        self.m.start(0, 1, TICKS)
        g.traffic_start(0, 1, TICKS)
        self.step = self.m.step

    def reads(self, g):
        return [(f"traffic_top by column {c}", g.traffic_top(TOP, c), self.m.top(TOP, c)) for c in range(_ffi.TRAFFIC_COLUMNS)]


class Tree(Churn):
    def __init__(self, o, g, n):
        self.entries = tr.churn_entries(n, FAN, TICKS)
        self.m = TreeModel(o)
        self.m.start(self.entries, 0, TICKS)
        g.tree_start(self.entries, 0, TICKS)
        self.step = self.m.step

    def reads(self, g):
        return [(f"tree_top of entry {e}", g.tree_top(e, TOP), self.m.top(e, TOP)) for e in range(len(self.entries))]


class Spread(Churn):
    def __init__(self, o, g, n):
        entries = tr.churn_entries(n, FAN, TICKS)
        self.m = SpreadModel(o)
        self.m.start(entries, 0, 1, TICKS)
        g.spread_start(entries, 0, 1, TICKS)
        self.step = self.m.step

    def reads(self, g):
        return [(f"spread_late by {by}", g.spread_late(TOP, by), self.m.late(TOP, by)) for by in SPREAD_BYS]


class Roll:
    """The roll ranks views, which the churn schedule (no SWIM layer: nobody notices a crash) leaves current: the ragged script
    of tests/test_observer_shapes.py, cut to 20 ticks — a crash at tick 4 under probe_interval 5, a leave, an event, a query."""
    @staticmethod
    def kw(n):
        return shapes.ragged_kw(n, FAN)

    @staticmethod
    def before(sim, n):
        pass

    @staticmethod
    def drive(sim, n, step):
        shapes.ragged_script(sim, n, no_tracker, step, 2 * TICKS)

    def __init__(self, o, g, n):
        self.o, self.step = o, o.step

    def reads(self, g):
        return [(f"roll_now by {by}", g.roll_now(TOP, by, nodes=True), RollModel(self.o).now(TOP, by, nodes=True)) for by in ROLL_BYS]


def compare(reads, what):
    for name, got, want in reads:
        if isinstance(want, tuple):
            same_now(got, want, f"{what}: {name}")
        else:
            same_records(got, want, f"{what}: {name}")


def tops(reads):
    """The rankings alone, as [top_k][words]."""
    return [words(want[1] if isinstance(want, tuple) else want).reshape(TOP, -1) for _, _, want in reads]


@pytest.mark.parametrize("n", (N, FEW))
@pytest.mark.parametrize("observer", (Traffic, Tree, Spread, Roll))
def test_rankings_of_64_before_and_behind_a_short_run(hiplib, observer, n):
    """Read right behind the start: every key ties — the meter's map is zero, no node has children, no entry of the spread map has
    started — so the ids ascend from 0, the first workgroup's before the second's, and the roll, whose score 0 means "not ranked",
    lists nobody.  Read again behind ten ticks of churn (the roll: twenty of the ragged script).  At three nodes 61 places stay unused."""
    kw = observer.kw(n)
    o, g = tt.make(n, kw), serf_amd.create(n, **kw)
    observer.before(o, n)
    observer.before(g, n)
    ob = observer(o, g, n)
    reads = ob.reads(g)
    compare(reads, f"{observer.__name__}({n}) at the start")
    for top in tops(reads):
        ids = (top[:, 0] & 0xFFFFFFFF).tolist()
        if observer is Roll:
            assert not top.any(), "the roll lists nobody and zeroes every place"
        elif observer is Spread:
            assert ids[:min(n, TOP)] == list(range(min(n, TOP))) and not top[:, 1:].any() and not top[n:].any(), "unused places are zero"
        else:
            assert ids == list(range(min(n, TOP))) + [NO_ID] * (TOP - min(n, TOP)), "unused places carry id 0xFFFFFFFF"
            assert not top[n:, 1:].any() and not (top[n:, 0] >> 32).any(), "... and zeros"
    observer.drive(o, n, ob.step)
    observer.drive(g, n, g.step)
    reads = ob.reads(g)
    compare(reads, f"{observer.__name__}({n}) behind the run")
    if observer is Roll:
        assert max(int(want[0]["listed"]) & 0xFFFFFFFF for _, _, want in reads) == (TOP if n == N else FEW - 1), "the run gave the roll nodes to list"
    elif n == N:
        assert any((top[:, 0] & 0xFFFFFFFF).tolist()[:8] != list(range(8)) for top in tops(reads)), "the run moved the ranking"
    assert g.digest() == o.digest()
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0, "the run stays inside the models' bounds"
    g.close()
    o.close()


def two_events(sim, step):
    """Node 0 injects an event, a tick goes by, it injects another, a tick goes by; returns their entries."""
    a = tr.inject_events(sim, (0,), 0x7700)
    step(1)
    b = tr.inject_events(sim, (0,), 0x7701)
    step(1)
    return a + b


@pytest.mark.parametrize("rank_by", SPREAD_BYS)
def test_spread_late_equal_scores_across_two_workgroups(hiplib, rank_by):
    """Nodes 1 .. 254 crash during ticks 0 .. 3; then node 0 injects two events, a tick apart.  Nodes 255 — the last lane of the
    first workgroup — and 256 — the only node of the second — run and get neither: missed 2, late_sum 0, the first key word equal,
    and the id alone puts 255 in front of 256.  Node 0, which has both, comes third; 61 places stay zero."""
    kw = tr.quiet_kw(N, FAN)
    scratch = tt.make(N, kw)
    entries = two_events(scratch, scratch.step)       # (nobody but node 0 touches node 0's event clock: crashes or none)
    scratch.close()
    o, g = tt.make(N, kw), serf_amd.create(N, **kw)
    m = SpreadModel(o)
    m.start(entries, 0, 1, 8)
    g.spread_start(entries, 0, 1, 8)
    for sim in (o, g):
        for x in range(1, N - 2):
            sim.inject(x // 64, _ffi.OP_CRASH, x)
    m.step(4)
    g.step(4)
    assert two_events(o, m.step) == entries and two_events(g, g.step) == entries
    want, every = m.late(TOP, rank_by, nodes=True)
    assert every["running"].nonzero()[0].tolist() == [0, N - 2, N - 1] and o.cluster_stats()["ops_dropped"] == 0
    assert every["missed"][[N - 2, N - 1]].tolist() == [2, 2] and every["late_sum"][[N - 2, N - 1]].tolist() == [0, 0]
    assert want["id"][:3].tolist() == [N - 2, N - 1, 0] and every["got"][0] == 2 and not words(want[3:]).any()
    got, gevery = g.spread_late(TOP, rank_by, nodes=True)
    same_records(gevery, every, f"rank_by {rank_by}: every node's record")
    same_records(got, want, f"rank_by {rank_by}: the ranking")
    assert g.digest() == o.digest()
    g.close()
    o.close()
