"""The delivery table (tests/delivery_table.py) against the oracle alone: is the table what it was meant to be?

Every variant tests/test_delivery_table_gpu.py runs is run here on the oracle — restore, one tick, three more — and the conditions
below are asserted.  None of them looks at the HIP library.
  1  every record arrives: a marker in every place of every case shows up at the case's node; the number of cases whose records
     change nothing at all is the one written down here
  2  every outcome class that exists for a record kind has a singles case
  3  order matters where it should: per trigger kind and placement a pair (A, B) in which B alone changes nothing and B after A
     does; a pair whose two orders end differently
  4  the known answers of tests/test_oracle_kat.py, literally, read through members / stats / dump
  5  stash pressure by construction (RF_STASH, RF_TMAX from serf_sim_tick.inc)
  6  tests/third_model.py agrees on the serf singles it can express
and every tag (a term of fast_noop / tail_retire / the walk) is reached true and false.
"""
import collections

import numpy as np
import pytest

from serf_amd import _ffi
from tests import delivery_table as dt
from tests import third_model as tm

# cases whose node ends the tick exactly as without their packets (expected no-ops), per variant: part of the table
EXPECTED_NOOPS = {"bijection-p4": 497, "bijection-p16": 375, "bijection-sharded": 497, "random-dense": 497, "random-sparse": 497, "random-ragged": 250,
                  "random-p8": 375, "random-small-0": 48, "random-small-1": 50, "random-small-2": 50, "random-small-3": 48, "random-small-4": 51,
                  "bijection-noswim": 673, "random-noswim": 673}
MARK = 1 << 20   # the markers' Lamport times: beyond every prepared clock, so a marker is never old and always advances the clock


class Run:
    """one variant on the oracle: the state of every node behind the first tick, with and without the packets in flight"""

    def __init__(self, oracle, name):
        self.b = b = dt.built(oracle, name)
        sim, ctl = dt.restored(oracle, b), dt.restored(oracle, b, b.control)
        self.before = dt.node_state(ctl, b.n)
        self.slot_of = ctl.dump(_ffi.ARR_SLOTMAP)
        for v in b.cases:
            sim.watch(v)
            ctl.watch(v)
        sim.step(1)
        ctl.step(1)
        self.after, self.ctl = dt.node_state(sim, b.n), dt.node_state(ctl, b.n)
        self.stats = {v: sim.stats(v) for v, c in b.cases.items() if c.kat}
        self.stats0 = {v: ctl.stats(v) for v, c in b.cases.items() if c.kat}
        self.members = {v: sim.members(v) for v, c in b.cases.items() if c.kat}
        self.events = sim.drain_events()
        self.classes = {v: dt.classify(c, self.after, self.ctl) for v, c in b.cases.items()}
        sim.step(3)
        self.final_digest = sim.digest()
        self.cluster = sim.cluster_stats()

    def gained(self, v):
        """the queue records the node has with its packets and not without, as a multiset"""
        def bag(q):
            live = q[q["meta"] != 0xFFFFFFFF]
            return collections.Counter((int(r["key"]), int(r["meta"] >> 4) & 15, int(r["val"])) for r in live)
        return bag(self.after["queue"][v]) - bag(self.ctl["queue"][v])

    def entry(self, v, x, which="after"):
        return getattr(self, which)["view"][v][self.slot_of[x]]

    def signature(self, c):
        """what the case's records did, comparable between nodes: the subject's entry, the row's changes, the broadcasts gained"""
        v = c.node
        e = self.entry(v, c.x)
        r1, r0 = self.after["rows"][v], self.ctl["rows"][v]
        row = tuple(int(r1[f]) - int(r0[f]) for f in ("clock", "n_known", "n_failed", "n_left", "inc", "overflow"))
        q = tuple(sorted(("X" if key == c.x else key, k, val) for (key, k, val), m in self.gained(v).items() for _ in range(m)))
        return (int(e["ltime"]), int(e["inc"]), int(e["bits"]), tuple(int(x) for x in e["conf"]), row, q)


_runs = {}


@pytest.fixture(scope="module")
def run(oracle):
    def get(name):
        if name not in _runs:
            _runs[name] = Run(oracle, name)
        return _runs[name]
    return get


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", list(dt.VARIANTS))
def test_every_place_of_every_case_is_delivered(oracle, run, name):
    r = run(name)
    b = r.b
    image = b.image.copy()
    _, at, nbytes = dt.sections(image)["inbox"]
    PG = max(1, b.kw["pkt_records"] // 4)
    inbox = np.zeros((b.kw["fanout"] * PG, b.n), _ffi.PACKET_DTYPE)
    want = {}
    for v, c in b.cases.items():
        for i, (pk, pg, pos, _) in enumerate(c.arrivals):
            k, col = b.rows[v][pk]
            rec = (dt.EVENT, 0x40000000 + 64 * v + i, MARK + i, 0)
            dt.put(inbox, k * PG + pg, col, pos, rec)
            want.setdefault(v, []).append(rec)
    image[at:at + nbytes] = inbox.view(np.uint8).reshape(-1)
    sim = dt.restored(oracle, b, image)
    sim.step(1)
    rows, queue = sim.dump(_ffi.ARR_ROWS), sim.dump(_ffi.ARR_QUEUE).reshape(b.n, _ffi.Q)
    for v, c in b.cases.items():
        if c.state.get("down"):
            assert rows[v]["event_clock"] < MARK, f"a process that is down received something: {c.describe()}"
            continue
        assert c.arrivals, c.describe()
        assert rows[v]["event_clock"] == MARK + len(want[v]), f"the markers arrive in order: {c.describe()}"
        have = dt.queue_set(queue[v])
        lost = [m for m in want[v][:40] if (m[1], m[0], m[2]) not in have]
        assert not lost, f"{len(lost)} of {len(want[v])} places were not delivered: {c.describe()}"
    touched = set(np.flatnonzero(rows["event_clock"] >= MARK))
    assert touched <= set(b.cases), "nodes without a case receive nothing"


@pytest.mark.parametrize("name", list(dt.VARIANTS))
def test_expected_noops_are_the_ones_written_down(run, name):
    r = run(name)
    noops = sorted(c.name for v, c in r.b.cases.items() if r.classes[v] == {"nothing"})
    print(f"{name}: {len(r.b.cases)} cases, {len(noops)} change nothing")
    assert all(r.classes[v] == {"nothing"} for v, c in r.b.cases.items() if c.noop), "a case recorded as a no-op did something"
    assert len(noops) == EXPECTED_NOOPS[name], f"{name}: {len(noops)} cases change nothing, the table says {EXPECTED_NOOPS[name]}"


# ------------------------------------------------------------------------------------------------ 2
SINGLES_IN = {"bijection": ("bijection-p4",), "random": ("random-dense",), "small": tuple(f"random-small-{i}" for i in range(5))}


@pytest.mark.parametrize("where", list(SINGLES_IN))
def test_every_outcome_class_has_a_singles_case_per_kind(run, where):
    seen = collections.defaultdict(collections.Counter)
    for name in SINGLES_IN[where]:
        r = run(name)
        for v, c in r.b.cases.items():
            if c.table == "singles" and len(c.arrivals) == 1:
                for cl in r.classes[v]:
                    seen[c.arrivals[0][3][0]][cl] += 1
    print({dt.KIND_NAME[k]: dict(cnt) for k, cnt in seen.items()})
    for kind, classes in dt.EXPECTED_CLASSES.items():
        missing = [cl for cl in classes if not seen[kind][cl]]
        assert not missing, f"{where}: no {dt.KIND_NAME[kind]} case ends in {missing}"


# ------------------------------------------------------------------------------------------------ 3
def pair_singles(oracle):
    """every (pair state, pair record) alone: what B does by itself"""
    if "pair-singles" not in dt._built:
        cases = [dt.Case("singles", f"s{si}/{dt.rname(a)}", dict(st, clock=20), [a]) for si, st in enumerate(dt.PAIR_STATES) for a in dt.PAIR_RECORDS]
        dt._built["pair-singles"] = dt.build(oracle, cases, 128)
    if "pair-singles" not in _runs:
        _runs["pair-singles"] = Run(oracle, "pair-singles")
    return _runs["pair-singles"]


@pytest.mark.parametrize("name,places", [("bijection-p4", dt.ONE_PAGE), ("random-dense", dt.ONE_PAGE), ("bijection-p16", dt.PLACES), ("random-p8", dt.PLACES)])
def test_order_matters_where_it_should(oracle, run, name, places):
    alone = pair_singles(oracle)
    single = {c.name: (alone.classes[v], alone.signature(c)) for v, c in alone.b.cases.items()}
    r = run(name)
    sig = {(c.name, c.place): r.signature(c) for v, c in r.b.cases.items() if c.table == "pairs" and not c.name.startswith("ragged")}
    found = collections.defaultdict(list)
    differ = []
    for (pname, place), s in sig.items():
        st, ab = pname.split("/", 1)
        a, bb = ab.split(">", 1)
        cls_b, _ = single[f"{st}/{bb}"]
        _, sig_a = single[f"{st}/{a}"]
        trig = "ALIVE" if a.startswith("ALIVE") else "LEAVEp" if a.startswith("LEAVEp") else None
        if trig and cls_b == {"nothing"} and s != sig_a:
            found[(trig, place)].append(pname)
        rev = sig.get((f"{st}/{bb}>{a}", place))
        if rev is not None and rev != s:
            differ.append((pname, place))
    print({k: len(v) for k, v in found.items()}, "pairs whose orders differ:", len(differ))
    for trig in ("ALIVE", "LEAVEp"):
        for place in places:
            assert found[(trig, place)], f"{name}: no pair after a {trig} trigger, placed as `{place}`, whose second record was a no-op alone and is not after it"
    assert differ, "no pair whose two orders end in different states"


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("name", ["bijection-p4", "random-dense", "bijection-noswim"])
def test_known_answers(run, name):
    r = run(name)
    kats = [c for c in r.b.cases.values() if c.kat]
    assert len(kats) >= 21
    for c in kats:
        v, ex, what = c.node, c.expect, f"{c.kat}: {c.describe()}"
        st, lt = r.members[v]
        incoming = collections.Counter((key, k, val) for _, _, _, (k, key, val, f) in c.arrivals)
        if "member" in ex:
            assert (int(st[c.x]), int(lt[c.x])) == ex["member"], what
        if "own" in ex:
            assert (int(st[v]), int(lt[v])) == ex["own"], what
        if "clock" in ex:
            assert r.stats[v].member_time == ex["clock"], what
        if "query_clock" in ex:
            assert r.stats[v].query_time == ex["query_clock"], what
        if "intent_queue" in ex:
            assert r.stats[v].intent_queue - r.stats0[v].intent_queue == ex["intent_queue"], what
        if "failed" in ex:
            assert (r.stats[v].failed, r.stats[v].left) == (ex["failed"], ex["left"]), what
        if "members_delta" in ex:
            assert int(r.stats[v].members) - int(r.stats0[v].members) == ex["members_delta"], what
        if "rebroadcasts" in ex:
            g = r.gained(v)
            assert sum((g & incoming).values()) == ex["rebroadcasts"] and sum(g.values()) == ex["rebroadcasts"], what
        if "intent" in ex:
            e = r.entry(v, c.x)
            have = None if (int(e["bits"]) & 1) or not (int(e["bits"]) >> 6) & 3 else ((int(e["bits"]) >> 6) & 3, int(e["ltime"]))
            assert have == ex["intent"], what
        if "events" in ex:
            assert [e[3] for e in r.events if e[1] == v and e[2] == _ffi.EV_USER] == ex["events"], what


# ------------------------------------------------------------------------------------------------ 5
def wave_counts(b):
    """per wave of 64 nodes: packets, records, records that advance the receiver's clock (never retired)"""
    n_w = (b.n + 63) // 64
    packets, records, adv = np.zeros(n_w, int), np.zeros(n_w, int), np.zeros(n_w, int)
    for v in range(b.n):
        packets[v // 64] += len(b.rows[v])
    return packets, records, adv


def test_stash_pressure_by_construction(oracle, run):
    cap = dt.caps()
    for name, dense in (("random-dense", True), ("random-sparse", False)):
        r = run(name)
        b = r.b
        packets, records, adv = wave_counts(b)
        rows = r.before["rows"]
        for v, c in b.cases.items():
            for _, _, _, (kind, key, val, f) in c.arrivals:
                records[v // 64] += 1
                clk = {dt.EVENT: "event_clock", dt.QUERY: "query_clock", dt.JOIN: "clock", dt.LEAVE: "clock"}.get(kind)
                if clk and val >= rows[v][clk] and (rows[v]["flags"] & 1):
                    adv[v // 64] += 1
        print(f"{name}: per wave packets max {packets.max()}, records max {records.max()} mean {records.mean():.1f}, advancing max {adv.max()}; RF_STASH {cap['RF_STASH']}, RF_TMAX {cap['RF_TMAX']}")
        assert packets.max() <= cap["RF_TMAX"], "no wave receives more packets than the tables hold"
        assert b.n % 64 == 0
        if dense:
            assert adv.max() > cap["RF_STASH"], "one whole wave has more records that can never be retired than the stash holds"
        else:
            assert records.max() <= cap["RF_STASH"], "no wave of the sparse layout overflows the stash"


# ------------------------------------------------------------------------------------------------ 6
def third_model_node(c, before, slot_of, n):
    """the case's prior state as a third_model.Node, or None where the module has no way to express it"""
    st = c.state
    if st.get("swim") or st.get("down") or "noslot" in (st.get("member"),) or st.get("filt") or st.get("flood"):
        return None
    if "ring" in st and st["ring"][1] in ("full", "ovf"):
        return None   # the overflow rows and the counted drop are model bounds: the third model's buckets are unbounded lists
    v = c.node
    nd = tm.Node(v, n, dt.RING, dt.RING, True)
    row = before["rows"][v]
    nd.clock.v, nd.event_clock.v, nd.query_clock.v = int(row["clock"]), int(row["event_clock"]), int(row["query_clock"])
    nd.event_min, nd.query_min = int(row["event_min"]), int(row["query_min"])
    nd.state = (int(row["flags"]) >> 1) & 3
    for x in set(dt.POOL) | {v}:
        if slot_of[x] == 0xFFFFFFFF:
            continue
        e = before["view"][v][slot_of[x]]
        bits = int(e["bits"])
        if bits & 1:
            nd.members[x] = [(bits >> 1) & 7, int(e["ltime"])]
        else:
            nd.members.pop(x, None)
            if (bits >> 6) & 3:
                nd.intents[x] = [(bits >> 6) & 3, int(e["ltime"])]
    for ring, buf in (("ering", nd.event_buf), ("qring", nd.query_buf)):
        for i in range(dt.RING):
            bk = before[ring][v][1 + i]
            if bk["keys"][0]:
                buf[i] = [int(bk["ltime"]), [int(k) for k in bk["keys"] if k]]
    return nd


def test_third_model_agrees_on_serf_singles(run):
    r = run("bijection-p4")
    serf = [c for c in r.b.cases.values() if c.table == "singles" and all(a[3][0] <= dt.QUERY for a in c.arrivals)]
    fed = 0
    for c in serf:
        nd = third_model_node(c, r.before, r.slot_of, r.b.n)
        if nd is None:
            continue
        fed += 1
        v = c.node
        for _, _, _, (kind, key, val, flags) in c.arrivals:
            nd.notify(kind, key, val, flags)
        what = c.describe()
        row = r.after["rows"][v]
        assert (nd.clock.v, nd.event_clock.v, nd.query_clock.v) == (int(row["clock"]), int(row["event_clock"]), int(row["query_clock"])), what
        for x in {c.x, v} - {None, dt.NOSLOT_ID}:
            if r.slot_of[x] == 0xFFFFFFFF:
                continue   # (no view slot: the entry is the baseline's, which nothing changes)
            e = r.entry(v, x)
            bits = int(e["bits"])
            have = [(bits >> 1) & 7, int(e["ltime"])] if bits & 1 else None
            assert nd.members.get(x) == have, what
        assert collections.Counter((key, k, val) for k, key, val in nd.rebroadcast) == r.gained(v), what
    print(f"third model: {fed} of {len(serf)} serf singles")
    assert 4 * fed >= 3 * len(serf), "the third model reaches fewer than three quarters of the serf singles"


# ------------------------------------------------------------------------------------------------ tags
def test_every_tag_has_both_polarities(run):
    seen = collections.defaultdict(lambda: collections.defaultdict(int))
    for name in ("bijection-p4", "random-dense"):
        for c in run(name).b.cases.values():
            for tag, pol in c.tags.items():
                for p in pol:
                    seen[tag][p] += 1
    print({t: dict(p) for t, p in sorted(seen.items())})
    assert len(seen) >= 20
    for tag, pol in seen.items():
        assert pol[True] and pol[False], f"tag {tag} is reached only with {dict(pol)}"


@pytest.mark.parametrize("name", ["bijection-p4", "random-dense", "random-sparse"])
def test_a_record_the_tags_retire_changes_nothing(run, name):
    """the count tests/test_delivery_table_gpu.py holds the classification to (delivery_table.verdict) never retires a record that
    does something: a singles case whose record it retires ends the tick as without its packets"""
    r = run(name)
    retired = 0
    for v, c in r.b.cases.items():
        if c.table == "singles" and len(c.arrivals) == 1 and not c.handled[0]:
            retired += 1
            assert r.classes[v] == {"nothing"}, c.describe()
    assert retired >= 150
