"""The HIP library against the delivery table (tests/delivery_table.py): every node of a cluster is one case — a prepared state
and the records travelling towards it — restored from the same image into a HIP handle and an oracle handle and delivered by the
tick kernel's own receive path: fast_noop / fast_retire / tail_retire, the balanced classification with its stash, `reload` and
the trigger walk under kRandomNodes, the per-page `slow` mask with its re-listing on the bijection path.  One tick, compared in
full; three more, compared by digest; then everything.  A difference is reported as the CASE of the first differing node.
(tests/test_delivery_table.py shows, on the oracle alone, that the table reaches what it is meant to reach.)"""
import ctypes as C
import os

import pytest

from serf_amd import _ffi
from tests import _scenario as sc
from tests import delivery_table as dt

pytestmark = pytest.mark.gpu

PER_NODE = {"rows": lambda i, n: i, "queue": lambda i, n: i // _ffi.Q, "inbox": lambda i, n: i % n, "view": lambda i, n: i % n,
            "event_ring": lambda i, n: i % n, "query_ring": lambda i, n: i % n}


def first_difference(g, o, built):
    """None, or a sentence that names the case of the first node at which the two handles differ"""
    for which, name in zip(sc.ARRAYS, sc.ARRAY_NAMES):
        a, b = g.dump(which), o.dump(which)
        assert a.shape == b.shape, f"{name} shape {a.shape} vs {b.shape}"
        i = sc.first_diff(a, b)
        if i is not None:
            if name not in PER_NODE:
                return f"{name}[{i}] differs: {a[i]} vs {b[i]}"
            v = PER_NODE[name](i, built.n)
            role = "sent by / addressed to" if name == "inbox" else "of"
            return f"{name}[{i}] {role} node {v} differs: HIP {a[i]} vs oracle {b[i]} -- {built.case_of(v)}"
    return None


def compare(g, o, built, what):
    if g.digest() != o.digest() or what == "final":
        d = first_difference(g, o, built)
        assert d is None, f"{what}: {d}"
        assert g.digest() == o.digest(), f"{what}: the digests differ although every array is the same"


def pair(oracle, hiplib, name):
    built = dt.built(oracle, name)
    g, o = dt.restored(hiplib, built), dt.restored(oracle, built)
    watched = sorted(built.cases)
    for v in watched:
        g.watch(v)
        o.watch(v)
    return built, g, o


@pytest.mark.parametrize("name", list(dt.VARIANTS))
def test_delivery_table(oracle, hiplib, name):
    built, g, o = pair(oracle, hiplib, name)
    assert g.tick == dt.T and g.digest() == o.digest(), "the restored image is the same state on both"
    g.step(1)
    o.step(1)
    d = first_difference(g, o, built)
    assert d is None, f"{name}, the tick that delivers the table: {d}"
    sc.assert_same_state(g, o, f"{name}: after the delivering tick")
    for t in range(3):
        g.step(1)
        o.step(1)
        compare(g, o, built, f"{name}: {t + 1} ticks after the delivery")
    compare(g, o, built, "final")
    sc.assert_same_state(g, o, f"{name}: final state")
    assert g.cluster_stats() == dict(o.cluster_stats(), events_lost=0), name
    eg, eo = g.drain_events(1 << 18), o.drain_events(1 << 18)
    if eg != eo:
        i = next((i for i, (a, b) in enumerate(zip(eg, eo)) if a != b), min(len(eg), len(eo)))
        v = (eg[i] if i < len(eg) else eo[i])[1]
        raise AssertionError(f"{name}: event {i} differs: HIP {eg[i:i + 1]} vs oracle {eo[i:i + 1]} -- {built.case_of(v)}")
    for q in built.queries:
        assert g.query_status(q) == o.query_status(q), f"{name}: query {q} (acks, responses, open)"
        for which in (0, 1):
            rg, ro = g.query_responders(q, which), o.query_responders(q, which)
            if rg != ro:
                v = sorted(set(rg) ^ set(ro))[0]
                raise AssertionError(f"{name}: query {q}, {'responses' if which else 'acks'} differ first at node {v} -- {built.case_of(v)}")


def test_four_ticks_in_one_step_call(oracle, hiplib):
    built = dt.built(oracle, "random-dense")
    a, b = dt.restored(hiplib, built), dt.restored(hiplib, built)
    a.step(4)
    for _ in range(4):
        b.step(1)
    assert a.tick == b.tick == dt.T + 4
    assert a.digest() == b.digest(), "one sim_step(4) and four sim_step(1) end in different states"


@pytest.fixture(scope="module")
def timing_lib(hiplib):
    """the instrumented build of the same source (-DTICK_TIMING, built next to the library): its tick kernel counts, per record kind,
    what the balanced classification leaves for the handlers"""
    import serf_amd
    path = os.path.splitext(serf_amd.LIB_PATH)[0] + "_timing.so"
    assert os.path.exists(path), f"{path} is not built"
    lib = _ffi.SimLib(path)
    lib.dll.sim_debug_timing.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    return lib


@pytest.mark.parametrize("name", ["random-dense", "random-sparse"])
def test_classification_leaves_exactly_the_records_it_should(oracle, timing_lib, name):
    """A verdict that retires LESS than fast_noop / tail_retire say changes no state — the handlers are always right — and shows only as
    work: the records left for the handlers, counted per kind by the instrumented kernel, against the count the table's tags give."""
    built = dt.built(oracle, name)
    want = dt.handled_by_kind(built)
    g, o = dt.restored(timing_lib, built), dt.restored(oracle, built)
    buf = (C.c_ulonglong * 32)()
    g.sync()
    assert timing_lib.dll.sim_debug_timing(buf, 1) == 0
    g.step(1)
    g.sync()
    assert timing_lib.dll.sim_debug_timing(buf, 1) == 0
    o.step(1)
    d = first_difference(g, o, built)
    assert d is None, f"{name}, instrumented build: {d}"
    got = {kind: int(buf[16 + kind]) for kind in want}
    print(name, "records left for the handlers:", {dt.KIND_NAME[k]: (got[k], want[k]) for k in want})
    for kind in want:
        if got[kind] != want[kind]:
            more = got[kind] > want[kind]
            some = [c.describe() for c in built.cases.values() for (_, _, _, rec), h in zip(c.arrivals, c.handled) if rec[0] == kind and bool(h) != more][:3]
            raise AssertionError(f"{name}: {got[kind]} {dt.KIND_NAME[kind]} records were left for the handlers, the table expects {want[kind]}; "
                                 f"{dt.KIND_NAME[kind]} cases expected to be {'retired' if more else 'handled'}, for example: " + " | ".join(some))
