"""The delivery table: a chosen record in front of a chosen state ON THE TICK'S RECEIVE PATH.

The tick kernel runs a handler for few records: fast_noop / fast_retire / tail_retire (serf_amd/csrc/serf_sim_handlers.inc) and,
under kRandomNodes, the balanced classification with its stash and its trigger walk (serf_amd/csrc/serf_sim_tick.inc) decide
which records change nothing.  This module builds clusters in which EVERY node is one case — a prepared state and 1 - 3 records
travelling towards it — as a checkpoint image: the states are set on a fresh oracle handle through its test hooks, the records
are written into the image's `inbox` section (the packets in flight), and sim_restore + one tick delivers them through the real
receive path of whichever implementation restores the image.

numpy, serf_amd._ffi and the oracle's hooks only: no GPU.  tests/test_delivery_table.py checks that the table is what it was
meant to be (against the oracle alone), tests/test_delivery_table_gpu.py runs the HIP library against it.
"""
import os
import re
from dataclasses import dataclass, field

import numpy as np

from serf_amd import _ffi
from tests import graph_model
from tests._oracle import Node
from tests.test_snapshot import sections

NONE, ALIVE, LEAVING, LEFT, FAILED = (_ffi.STATUS_NONE, _ffi.STATUS_ALIVE, _ffi.STATUS_LEAVING, _ffi.STATUS_LEFT, _ffi.STATUS_FAILED)
JOIN, LEAVE, EVENT, QUERY, AL, SUSPECT, DEAD = (_ffi.K_JOIN, _ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY, _ffi.K_ALIVE, _ffi.K_SUSPECT, _ffi.K_DEAD)
KIND_NAME = {JOIN: "JOIN", LEAVE: "LEAVE", EVENT: "EVENT", QUERY: "QUERY", AL: "ALIVE", SUSPECT: "SUSPECT", DEAD: "DEAD"}
LEN_BYTES = {JOIN: 16, LEAVE: 16, EVENT: 32, QUERY: 48, AL: 64, SUSPECT: 32, DEAD: 32}   # what the oracle's own senders put on the wire
PRUNE = 1

T = 10                 # the tick of the image: the packets in flight were "sent" during tick T - 1
RING = 16              # both de-dup rings; one overflow row each
VIEW_SLOTS = 96
HOST = 0               # the node whose (no-op) operations give the subjects their view slots; it has no case
ORIGIN = 1             # the origin of the running queries; no case either
POOL = (17, 33, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14)   # every subject is one of these; 17 and 33 share their low four bits
NOSLOT_ID = 40         # an id that is never given a view slot
CONF = (50, 51, 52, 53)   # the accusers the prepared suspicions are counted from
NEWCONF = 60           # an accuser nobody has counted
Q_RUN, Q_FILT = 7001, 7002   # running queries (ack + respond): without / with an id filter
L = 12                 # the prepared member time; incarnation 3 is the prepared incarnation
INC = 3
LR = 8                 # the Lamport time of the ring cases' records
QLT = 2                # the Lamport time of the running queries (the origin's query clock when it sends them)


def caps():
    """RF_STASH and RF_TMAX as serf_sim_tick.inc defines them"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "serf_amd", "csrc", "serf_sim_tick.inc")).read()
    return {name: int(re.search(r"#define\s+" + name + r"\s+(\d+)u", src).group(1)) for name in ("RF_STASH", "RF_TMAX")}


@dataclass
class Case:
    table: str                       # singles | pairs | triples
    name: str
    state: dict                      # see prepare()
    records: list                    # [(kind, key, val, flags)]; key "X" / "Y" / "SELF" is resolved when the case gets its node
    place: str = "page"              # page: one page of one packet | pages: consecutive pages of one packet | packets: one packet each
    kat: str = None                  # the reference test this case restates
    expect: dict = None              # ... and its literal answers
    noop: bool = False               # recorded as an expected no-op: condition 1 does not ask for a difference
    x: int = None                    # the subject (filled in by build)
    node: int = None
    arrivals: list = field(default_factory=list)   # (packet of the row, page, position, (kind, key, val, flags)) in arrival order
    tags: dict = field(default_factory=dict)       # term of fast_noop / tail_retire / the walk -> set of polarities seen
    handled: list = field(default_factory=list)    # per arrival: does the classification leave the record for a handler (see verdict())

    def need(self):
        return len(self.records) if self.place == "packets" else 1

    def pages(self):
        return len(self.records) if self.place == "pages" else 1

    def describe(self):
        rec = ", ".join(f"{KIND_NAME[k]}{'|F%d' % f if f else ''}(key {key}, val {val:#x})" for k, key, val, f in self.resolved())
        return f"case {self.table}/{self.name} at node {self.node}: state {self.state}, subject {self.x}; records [{rec}]; placement {self.place}"

    def resolved(self):
        sub = {"X": self.x, "SELF": self.node, "Y": 33 if self.x == 17 else 17}
        out = []
        for k, key, val, f in self.records:
            key = sub.get(key, key)
            if k in (SUSPECT, DEAD):   # val = (incarnation, from)
                inc, frm = val
                val = inc | (sub.get(frm, frm) << 32)
            out.append((k, key, QLT if val == "QLT" else val, f))
        return out


# ------------------------------------------------------------------------------------------------ the catalogue
MEMBER_STATES = ("noslot", "unknown", "ijoin", "ileave", "alive", "leaving", "left", "failed", "none")


def swim_states(kconf):
    return ["alive"] + [f"suspect{j}" for j in range(kconf + 1)] + ["resuspect", "dead", "swleft", "unknown", "noslot"]


def member_records():
    out = []
    for kind, flags in ((JOIN, 0), (LEAVE, 0), (LEAVE, PRUNE)):
        for lt in (L - 2, L, L + 2):
            out.append((kind, "X", lt, flags))
    return out


def swim_records():
    out = [(AL, "X", inc, 0) for inc in (INC - 1, INC, INC + 1)]
    # accusers: counted first, counted later (or a stale word of an earlier suspicion), new, the receiver, node 0 (an unused confirmer word is 0)
    out += [(SUSPECT, "X", (inc, frm), 0) for inc in (INC - 1, INC, INC + 1) for frm in (CONF[0], CONF[1], NEWCONF, "SELF", HOST)]
    out += [(DEAD, "X", (inc, frm), 0) for inc in (INC - 1, INC, INC + 1) for frm in ("X", NEWCONF)]
    return out


def rname(r):
    k, key, val, f = r
    return f"{KIND_NAME[k]}{'p' if (k == LEAVE and f) else ''}{':' + str(f) if (f and k != LEAVE) else ''}@{val if not isinstance(val, tuple) else '%d<%s' % val}"


def singles(kconf):
    out = []
    # member entry x intent record x (record time against the entry's) x (against the receiver's clock: the `adv` term)
    for st in MEMBER_STATES:
        for r in member_records():
            for clock in (1, 20):
                out.append(Case("singles", f"{st}/{rname(r)}/clock{clock}", dict(member=st, clock=clock), [r]))
    # memberlist state x memberlist record
    for st in swim_states(kconf):
        for r in swim_records():
            out.append(Case("singles", f"sw-{st}/{rname(r)}", dict(swim=st), [r]))
    # the receiver itself as the subject: refutations
    for serf in (0, 1):
        out.append(Case("singles", f"self/LEAVE@7/serf{serf}", dict(self_at=0, clock=1, serf=serf), [(LEAVE, "SELF", 7, 0)],
                        kat="base.rs:1470-1480, 381-397 (test_leave_intent_refute_self)" if serf == 0 else None,
                        expect=dict(clock=9, own=(ALIVE, 8), intent_queue=1) if serf == 0 else None))
    out.append(Case("singles", "self/LEAVE@0-old", dict(self_at=5, clock=9), [(LEAVE, "SELF", 5, 0)]))
    for inc in (0, 1):   # own incarnation is 0: an alive about self at <= and > it
        out.append(Case("singles", f"self/ALIVE@{inc}", dict(self_at=0), [(AL, "SELF", inc, 0)]))
    for kind in (SUSPECT, DEAD):
        for inc in (0, 2):
            out.append(Case("singles", f"self/{KIND_NAME[kind]}@{inc}", dict(self_at=0), [(kind, "SELF", (inc, NEWCONF), 0)]))
    # ring bucket of the record's Lamport time x key held / new x the record's time against the clock
    for kind in (EVENT, QUERY):
        for bucket in ("empty", "head", "tail", "ovf", "full", "lap"):
            for key in ("held", "new"):
                if bucket == "empty" and key == "held":
                    continue
                for rel, clock in (("outside", LR + 1 + 2 * RING + 3), ("below", LR + 3), ("equal", LR), ("above", LR - 2)):
                    out.append(Case("singles", f"{KIND_NAME[kind]}/{bucket}/{key}/{rel}", dict(ring=(kind, bucket), rclock=clock),
                                    [(kind, 900 if key == "held" else 990, LR, 0)]))
    # queries: flags, the id filter
    for flags in (_ffi.F_NO_BROADCAST, _ffi.F_ACK, _ffi.F_RESPOND, _ffi.F_ACK | _ffi.F_RESPOND):
        out.append(Case("singles", f"QUERY/running/flags{flags}", dict(), [(QUERY, Q_RUN, "QLT", flags)]))
    out.append(Case("singles", "QUERY/filter/inside", dict(filt=True), [(QUERY, Q_FILT, "QLT", _ffi.F_ACK | _ffi.F_RESPOND)]))
    out.append(Case("singles", "QUERY/filter/outside", dict(), [(QUERY, Q_FILT, "QLT", _ffi.F_ACK | _ffi.F_RESPOND)]))
    # the receiver as a whole
    for kind in (EVENT, QUERY):
        for what, lt in (("below", 4), ("above", 6)):
            out.append(Case("singles", f"{KIND_NAME[kind]}/mintime/{what}", dict(mintime=(kind, 5)), [(kind, 991, lt, 0)]))
            out.append(Case("singles", f"{KIND_NAME[kind]}/mintime/{what}/held", dict(mintime=(kind, 5), ring=(kind, "head-at", lt), rclock=lt + 3),
                            [(kind, 900, lt, 0)]))
    for serf in (1, 2):
        for r in ((JOIN, "X", L + 2, 0), (LEAVE, "X", L + 2, 0), (EVENT, 992, 3, 0), (AL, "X", INC + 1, 0)):
            out.append(Case("singles", f"serf{serf}/{rname(r)}", dict(member="alive", swim="alive", serf=serf), [r]))
    for r in ((JOIN, "X", L + 2, 0), (EVENT, 993, 3, 0), (QUERY, 994, 3, 0), (AL, "X", INC + 1, 0)):
        out.append(Case("singles", f"down/{rname(r)}", dict(member="alive", swim="alive", down=True), [r], noop=True))
    out += known_answers()
    return out


def known_answers():
    """tests/test_oracle_kat.py's arms, on the receive path; clocks start at 1 as in a fresh Serf"""
    K = lambda name, state, records, kat, expect, place="page": Case("singles", "kat/" + name, dict(state, clock=state.get("clock", 1)), records, place, kat, expect)   # noqa: E731
    J, Lv = (lambda lt: (JOIN, "X", lt, 0)), (lambda lt, p=0: (LEAVE, "X", lt, p))
    return [
        K("join-buffer-early", dict(member="unknown"), [J(10), J(10)], "join.rs:8-35 (test_join_intent_buffer_early)", dict(intent=(1, 10), rebroadcasts=1)),
        K("join-old-message", dict(member="alive"), [J(10)], "join.rs:38-85 (test_join_intent_old_message)", dict(member=(ALIVE, 12), rebroadcasts=0, intent=None)),
        K("join-newer", dict(member="alive"), [J(14)], "join.rs:88-134 (test_join_intent_newer)", dict(member=(ALIVE, 14), clock=15, rebroadcasts=1)),
        K("join-reset-leaving", dict(member="leaving"), [J(14)], "join.rs:137-185 (test_join_intent_reset_leaving)", dict(member=(ALIVE, 14), clock=15)),
        K("leave-buffer-early", dict(member="unknown"), [Lv(10), Lv(10)], "leave.rs:4-33 (test_leave_intent_buffer_early)", dict(intent=(2, 10), rebroadcasts=1)),
        K("leave-old-message", dict(member="alive"), [Lv(10)], "leave.rs:36-82 (test_leave_intent_old_message)", dict(member=(ALIVE, 12), rebroadcasts=0, intent=None)),
        K("leave-newer", dict(member="alive"), [Lv(14)], "leave.rs:85-136 (test_leave_intent_newer)", dict(member=(LEAVING, 14), clock=15, rebroadcasts=1)),
        K("leave-failed-to-left", dict(member="failed", mtime=3), [Lv(9)], "base.rs:1497-1569 (test_leave_intent_state_arms)", dict(member=(LEFT, 9), failed=0, left=1, rebroadcasts=1)),
        K("leave-left-same", dict(member="left", mtime=9), [Lv(9)], "base.rs:1497-1569 (test_leave_intent_state_arms: `<=`)", dict(member=(LEFT, 9), rebroadcasts=0)),
        K("leave-left-newer", dict(member="left", mtime=9), [Lv(10)], "base.rs:1512 (test_leave_intent_state_arms: Left stays Left)", dict(member=(LEFT, 10), rebroadcasts=1)),
        K("leave-none-arm", dict(member="none", mtime=1), [Lv(5)], "base.rs:1501 (test_leave_intent_state_arms: the None arm)", dict(member=(NONE, 5), rebroadcasts=0)),
        K("prune", dict(member="alive", mtime=2), [Lv(5, PRUNE)], "base.rs:1502-1511,1628-1653 (test_prune)", dict(member=(NONE, 0), members_delta=-1, rebroadcasts=1)),
        K("user-event-same-clock", dict(), [(EVENT, 101, 1, 0), (EVENT, 102, 1, 0), (EVENT, 103, 1, 0)], "event.rs:34-85 (test_user_event_same_clock)", dict(rebroadcasts=3, events=[101, 102, 103])),
        K("user-event-same-clock-dup", dict(ring=(EVENT, "three-at", 1), rclock=1), [(EVENT, 101, 1, 0), (EVENT, 102, 1, 0), (EVENT, 103, 1, 0)], "event.rs:34-85 (test_user_event_same_clock: duplicates)", dict(rebroadcasts=0), place="packets"),
        K("user-event-u1-same-key", dict(ring=(EVENT, "head-at", 3), rclock=1), [(EVENT, 900, 3 + RING, 0)], "base.rs:801-807 (test_user_event_quirk_u1)", dict(rebroadcasts=0)),
        K("user-event-u1-other-key", dict(ring=(EVENT, "head-at", 3), rclock=1), [(EVENT, 9, 3 + RING, 0)], "base.rs:801-807 (test_user_event_quirk_u1)", dict(rebroadcasts=1)),
        K("query-same-clock", dict(), [(QUERY, 1, 1, 0), (QUERY, 1, 1, 0)], "event.rs:674-772 (test_query_same_clock)", dict(rebroadcasts=1, query_clock=2)),
        K("query-no-broadcast", dict(), [(QUERY, 4, 1, _ffi.F_NO_BROADCAST)], "base.rs:1062-1066 (test_query_same_clock: F_NO_BROADCAST)", dict(rebroadcasts=0, query_clock=2)),
        K("query-q2", dict(ring=(QUERY, "head-at", 2), rclock=1), [(QUERY, 900, 2 + RING, 0), (QUERY, 900, 2 + RING, 0)], "base.rs:1027-1036 (test_query_quirks: Q2)", dict(rebroadcasts=2)),
        K("query-q1", dict(rclock=2 * RING + 2, ring=(QUERY, "none")), [(QUERY, 6, 2 * RING + 1, 0)], "base.rs:1012-1014 (test_query_quirks: Q1)", dict(rebroadcasts=0)),
    ]


PAIR_STATES = (dict(member="alive", swim="alive"), dict(member="alive", swim="suspect1"), dict(member="alive", swim="dead"),
               dict(member="alive", swim="swleft"), dict(member="unknown"), dict(member="ijoin"), dict(member="leaving", swim="alive"))
PAIR_RECORDS = ((JOIN, "X", L, 0), (JOIN, "X", L + 2, 0), (LEAVE, "X", L + 1, 0), (LEAVE, "X", L + 2, PRUNE), (AL, "X", INC, 0), (AL, "X", INC + 1, 0),
                (SUSPECT, "X", (INC, NEWCONF), 0), (SUSPECT, "X", (INC + 1, NEWCONF), 0), (DEAD, "X", (INC, NEWCONF), 0), (DEAD, "X", (INC + 1, "X"), 0))
PLACES = ("page", "pages", "packets")


def pairs(places=PLACES):
    out = []
    for si, st in enumerate(PAIR_STATES):
        for a in PAIR_RECORDS:
            for b in PAIR_RECORDS:
                for place in places:
                    # clock 20: a record is retired only when it does not advance the clock; the member records' times are all below it
                    out.append(Case("pairs", f"s{si}/{rname(a)}>{rname(b)}", dict(st, clock=20), [a, b], place))
    return out


def triples(places=PLACES, floods=0, fan=4, pkt_records=4):
    out = []
    ev = (EVENT, 995, 3, 0)
    trig = ((dict(member="alive", swim="dead", clock=20), (AL, "X", INC + 1, 0), (SUSPECT, "X", (INC + 1, NEWCONF), 0)),
            (dict(member="alive", swim="dead", clock=20), (AL, "X", INC + 1, 0), (JOIN, "X", L, 0)),
            (dict(member="alive", swim="alive", clock=20), (LEAVE, "X", L + 2, PRUNE), (JOIN, "X", L, 0)),
            (dict(member="alive", swim="alive", clock=20), (LEAVE, "X", L + 2, PRUNE), (LEAVE, "X", L, 0)),
            (dict(member="alive", swim="swleft", clock=20), (AL, "X", INC + 1, 0), (DEAD, "X", (INC + 1, NEWCONF), 0)))
    for i, (st, a, b) in enumerate(trig):
        for place in places:
            out.append(Case("triples", f"trigger{i}/{rname(a)},EVENT,{rname(b)}", st, [a, ev, b], place))
        # the same low four bits, another subject: the walk lists it conservatively and nothing may change for it
        for place in places:
            if place == "pages":
                continue
            y = (b[0], "Y", b[2] if not isinstance(b[2], tuple) else (INC - 1, b[2][1]), b[3])
            if b[0] in (JOIN, LEAVE):
                y = (b[0], "Y", 1, b[3])   # every member is Alive @ 1 in the baseline: a no-op against Y
            out.append(Case("triples", f"collide{i}/{rname(a)},{rname(y)}", dict(st, x17=True), [a, y], place))
    for i in range(floods):   # every record of every packet queues a broadcast: `pend` at its maximum, the queue pushed beyond SIM_Q_HOT
        out.append(Case("triples", f"flood{i}", dict(flood=True, clock=1), [], "flood"))
    return out


def table(kconf, places=PLACES, floods=0, only=("singles", "pairs", "triples")):
    out = []
    if "singles" in only:
        out += singles(kconf)
    if "pairs" in only:
        out += pairs(places)
    if "triples" in only:
        out += triples(places, floods)
    return out


# ------------------------------------------------------------------------------------------------ states
def kconf_of(oracle, sim):
    import ctypes as C
    k, Tm = C.c_uint32(), (C.c_uint32 * 4)()
    assert oracle.t["swim_params"](sim.h, C.byref(k), Tm) == 0
    return k.value


def prepare(oracle, sim, case, swim_on):
    """the case's prior state at its node, through the oracle's hooks (n_known / failed / left and the timers stay consistent)"""
    nd, st, x = Node(oracle, sim, case.node), case.state, case.x
    t = oracle.t
    mt = st.get("mtime", L)
    m = st.get("member")
    if m == "unknown":
        nd.leave_intent(x, 2, prune=True)            # erased: the slot is there, the member is not
    elif m in ("ijoin", "ileave"):
        nd.leave_intent(x, 2, prune=True)
        assert nd.upsert_intent(x, Node.JOIN if m == "ijoin" else Node.LEAVE, mt)
    elif m in ("alive", "leaving", "left", "failed", "none"):
        nd.set_member(x, dict(alive=ALIVE, leaving=LEAVING, left=LEFT, failed=FAILED, none=NONE)[m], mt, stamp=T)
    if "self_at" in st:
        nd.set_member(case.node, ALIVE, st["self_at"])
    sw = st.get("swim")
    if sw and swim_on and sw not in ("noslot",):
        if sw == "unknown":
            nd.leave_intent(x, 2, prune=True)
        else:
            if sw == "resuspect":   # an earlier suspicion with every confirmer, refuted, then a new one: what do the confirmer words hold?
                nd.alive(x, INC - 1)
                for j in range(4):
                    nd.suspect(x, INC - 1, CONF[j])
                nd.alive(x, INC)
                nd.suspect(x, INC, CONF[0])
            else:
                nd.alive(x, INC)
            if sw.startswith("suspect"):
                for j in range(int(sw[7:]) + 1):
                    nd.suspect(x, INC, CONF[j])
            elif sw == "dead":
                nd.dead(x, INC, CONF[0])
            elif sw == "swleft":
                nd.dead(x, INC, x)
    if "ring" in st:
        kind, bucket = st["ring"][0], st["ring"][1]
        push = nd.user_event if kind == EVENT else nd.query
        nd.set_clock(Node.EVENT if kind == EVENT else Node.QUERY, 1)
        if bucket == "head-at":
            push(900, st["ring"][2])
        elif bucket == "three-at":
            for key in (101, 102, 103):
                push(key, st["ring"][2])
        elif bucket == "lap":
            push(900, LR + RING)
        elif bucket not in ("empty", "none"):
            fill = dict(head=[900, 901], tail=[801, 802, 803, 900], ovf=[801, 802, 803, 804, 805, 806, 807, 900],
                        full=[801, 802, 803, 804, 805, 806, 807, 808, 809, 810, 811, 900])[bucket]
            for key in fill:
                push(key, LR)
    if st.get("flood"):
        for i in range(3):
            nd.user_event(700 + i, 1)
    which = {EVENT: 1, QUERY: 2}
    if "mintime" in st:
        assert t["set_min_time"](sim.h, case.node, which[st["mintime"][0]], st["mintime"][1]) == 0
    if "clock" in st:
        nd.set_clock(Node.CLOCK, st["clock"])
    if "rclock" in st:
        nd.set_clock(Node.EVENT, st["rclock"])
        nd.set_clock(Node.QUERY, st["rclock"])
    if "serf" in st:
        assert t["set_serf_state"](sim.h, case.node, st["serf"]) == 0
    if st.get("down"):
        sim.inject(T, _ffi.OP_CRASH, case.node)


# ------------------------------------------------------------------------------------------------ the image
def put(inbox, cell, node, pos, rec):
    kind, key, val, flags = rec
    v48 = ((val & 0xFFFFFF) | (((val >> 32) & 0xFFFFFF) << 24)) if kind in (SUSPECT, DEAD) else (val & 0xFFFFFFFFFFFF)
    len64 = (LEN_BYTES[kind] + 15) // 16
    assert inbox["hi_meta"][cell, node, pos] == 0, "one record per place"
    inbox["key"][cell, node, pos] = key
    inbox["val_lo"][cell, node, pos] = v48 & 0xFFFFFFFF
    inbox["hi_meta"][cell, node, pos] = ((v48 >> 32) << 16) | ((63 - len64) << 8) | (kind << 4) | flags


@dataclass
class Built:
    image: np.ndarray
    control: np.ndarray              # the same image with nothing in flight
    cases: dict                      # node -> Case
    n: int
    kw: dict
    rows: list                       # node -> its packets in arrival order: (inbox slot k, column)
    kconf: int
    queries: tuple = (Q_RUN, Q_FILT)

    def case_of(self, node):
        c = self.cases.get(int(node))
        return c.describe() if c else f"node {int(node)} (lane {int(node) % 64} of wave {int(node) // 64}) has no case"

    def config(self):
        return _ffi.make_config(self.n, **self.kw)


def build(oracle, cases, n, fan=4, layout="dense", random_fanout=False, last_wave=(), **cfg):
    """(image, the case of every node, the records of every case in the order they will arrive) as a Built.  `cases`: a list from
    table(); `layout`: dense — a case on every lane; sparse — on every fourth lane.  `last_wave`: cases for the last nodes."""
    kw = dict(fanout=fan, view_slots=VIEW_SLOTS, event_ring=RING, query_ring=RING, ring_overflow=1, probe_interval=5, leave_delay=6,
              pkt_records=4)
    kw.update(cfg)
    if random_fanout:
        kw["flags"] = _ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT
    swim_on = kw["probe_interval"] > 0
    PG = max(1, kw["pkt_records"] // 4)
    sim = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    assert oracle.t["set_tick"](sim.h, T) == 0
    feff = graph_model.feff_of(n, fan)
    if random_fanout:
        rcsr, rsrc = graph_model.one_handle(int(sim.cfg.seed), T - 1, n, feff)
        rows = [[(int(p) & 3, int(p) >> 2) for p in rsrc[rcsr[v]:rcsr[v + 1]]] for v in range(n)]
    else:
        rows = [[(k, v) for k in range(feff)] for v in range(n)]
    # cases to nodes, by the in-degree and the pages they need; the flood cases: the even lanes of wave 1
    step = 4 if layout == "sparse" else 1
    free = [v for v in range(2, n - len(last_wave), step) if v != NOSLOT_ID]
    by_need = {}
    for c in cases:
        if c.pages() > PG:
            continue
        by_need.setdefault("flood" if c.place == "flood" else c.need(), []).append(c)
    for q in by_need.values():
        q.reverse()
    placed = {}
    for v in free:
        deg = len(rows[v])
        if by_need.get("flood") and 64 <= v < 128 and v % 2 == 0 and deg >= 2:
            c = by_need["flood"].pop()
        else:
            c = next((by_need[k].pop() for k in (3, 2, 1) if k <= deg and by_need.get(k)), None)
        if c is not None:
            placed[v] = c
    for i, c in enumerate(last_wave):
        v = n - len(last_wave) + i
        assert len(rows[v]) >= c.need(), f"node {v} receives {len(rows[v])} packets, its case needs {c.need()}"
        placed[v] = c
    left = sum(len(q) for q in by_need.values())
    assert left == 0, f"{left} cases found no node: a larger cluster is needed"
    # subjects and view slots: a join intent at Lamport time 0 delivered to HOST is a no-op there (it knows every member Alive @ 1);
    # scheduling the delivery is what hands out the subject's slot
    slots = list(POOL) + list(CONF) + [NEWCONF]
    pool_x = [p for p in POOL if p not in (17, 33)]
    for i, (v, c) in enumerate(sorted(placed.items())):
        c.node = v
        c.x = NOSLOT_ID if "noslot" in (c.state.get("member"), c.state.get("swim")) else 17 if c.state.get("x17") else (pool_x + [17, 33])[i % len(POOL)]
        if c.x == v:
            c.x = 5 if v != 5 else 6
        if "self_at" in c.state or any(r[1] == "SELF" for r in c.records) or (c.state.get("down") and swim_on):
            slots.append(v)
    seen = set()
    for s in slots:
        if s not in seen:
            seen.add(s)
            sim.inject_record(T, HOST, s, (63 - 1) << 18 | JOIN << 4, 0)   # a join intent at Lamport time 0 about a member HOST knows: a no-op
    assert len(seen) <= VIEW_SLOTS
    # the running queries, so that acks and responses are counted
    Node(oracle, sim, ORIGIN).set_clock(Node.QUERY, QLT)
    sim.query(ORIGIN, Q_RUN, _ffi.F_ACK | _ffi.F_RESPOND)
    filt = [v for v, c in placed.items() if c.state.get("filt")][:_ffi.QF_IDS]
    sim.query(ORIGIN, Q_FILT, _ffi.F_ACK | _ffi.F_RESPOND, ids=filt or [ORIGIN])
    for v, c in sorted(placed.items()):
        prepare(oracle, sim, c, swim_on)
    image = sim.snapshot()
    sec = sections(image)
    _, at, nbytes = sec["inbox"]
    assert nbytes == fan * PG * n * _ffi.PACKET_DTYPE.itemsize
    inbox = np.zeros((fan * PG, n), _ffi.PACKET_DTYPE)
    control = image.copy()
    control[at:at + nbytes] = inbox.view(np.uint8).reshape(-1)
    nflood = 0
    for v, c in sorted(placed.items()):
        if c.place == "flood":
            recs = [(EVENT, 100000 + 64 * v + i, 1 + i % 3, 0) for i in range(4 * PG * len(rows[v]))]
            where = [(i // (4 * PG), (i // 4) % PG, i % 4) for i in range(len(recs))]
            nflood += 1
        else:
            recs = c.resolved()
            if c.place == "page":
                first = 0 if len(recs) == 3 else (v % 2)
                where = [(0, 0, first + (2 if len(recs) == 2 else 1) * i) for i in range(len(recs))]
            elif c.place == "pages":
                where = [(0, i, (v + i) % 4) for i in range(len(recs))]
            else:
                where = [(i, 0, (v + 2 * i) % 4) for i in range(len(recs))]
        for (pk, pg, pos), rec in zip(where, recs):
            k, col = rows[v][pk]
            put(inbox, k * PG + pg, col, pos, rec)
            c.arrivals.append((pk, pg, pos, rec))
        c.arrivals.sort(key=lambda a: a[:3])
    image[at:at + nbytes] = inbox.view(np.uint8).reshape(-1)
    b = Built(image, control, placed, n, kw, rows, kconf_of(oracle, sim))
    tag_cases(oracle, sim, b)
    return b


def restored(lib, built, image=None):
    sim = _ffi.Sim(lib, built.config())
    sim.restore(built.image if image is None else image)
    return sim


# ------------------------------------------------------------------------------------------------ reading a handle
def node_state(sim, n):
    """{array: [n][...]}: every state array indexed by node, for diffs node by node"""
    rows = sim.dump(_ffi.ARR_ROWS)
    queue = sim.dump(_ffi.ARR_QUEUE).reshape(n, _ffi.Q)
    view = sim.dump(_ffi.ARR_VIEW).reshape(-1, n)
    er = sim.dump(_ffi.ARR_ERING).reshape(-1, n)
    qr = sim.dump(_ffi.ARR_QRING).reshape(-1, n)
    return dict(rows=rows, queue=queue, view=view.T, ering=er.T, qring=qr.T)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


EXPECTED_CLASSES = {JOIN: ("nothing", "clock", "entry", "rebroadcast"),
                    LEAVE: ("nothing", "clock", "entry", "rebroadcast", "refute", "erased"),
                    EVENT: ("nothing", "clock", "entry", "rebroadcast", "overflow"),
                    QUERY: ("nothing", "clock", "entry", "rebroadcast", "overflow"),
                    AL: ("nothing", "entry", "rebroadcast", "refute"),
                    SUSPECT: ("nothing", "entry", "rebroadcast", "refute"),
                    DEAD: ("nothing", "entry", "rebroadcast", "refute")}


def queue_set(q):
    live = q[q["meta"] != 0xFFFFFFFF]
    return {(int(r["key"]), int(r["meta"] >> 4) & 15, int(r["val"])) for r in live}


def classify(case, with_, ctl):
    """the outcome classes of one case: its node after the tick with and without its packets"""
    v = case.node
    out = set()
    r1, r0 = with_["rows"][v], ctl["rows"][v]
    clocks = any(r1[f] != r0[f] for f in ("clock", "event_clock", "query_clock"))
    rest = any(np.any(r1[f] != r0[f]) for f in r1.dtype.names if f not in ("clock", "event_clock", "query_clock"))
    entry = any((raw(with_[k][v:v + 1]) != raw(ctl[k][v:v + 1])).any() for k in ("view", "ering", "qring"))
    gained = queue_set(with_["queue"][v]) - queue_set(ctl["queue"][v])
    queue = (raw(with_["queue"][v:v + 1]) != raw(ctl["queue"][v:v + 1])).any()
    if r1["overflow"] != r0["overflow"]:
        out.add("overflow")
    if entry:
        out.add("entry")
    if r1["n_known"] < r0["n_known"]:
        out.add("erased")
    incoming = {(key, k, val) for _, _, _, (k, key, val, f) in case.arrivals}
    if gained & incoming:
        out.add("rebroadcast")
    if any(key == v and k in (JOIN, AL) for key, k, val in gained - incoming):
        out.add("refute")
    if not out and not rest and not queue:
        out.add("clock" if clocks else "nothing")
    return out


# ------------------------------------------------------------------------------------------------ tags: which term, which polarity
def tag_cases(oracle, sim, built):
    """Per case and record: the terms of fast_noop / fast_retire / tail_retire / the trigger walk, evaluated on the prepared state
    (the entry as the oracle holds it before the tick).  A restatement for BOOKKEEPING only — which cases reach a term true and
    which false; nothing is asserted about the library from it."""
    n, kconf = built.n, built.kconf
    rows = sim.dump(_ffi.ARR_ROWS)
    er = sim.dump(_ffi.ARR_ERING).reshape(-1, n)
    qr = sim.dump(_ffi.ARR_QRING).reshape(-1, n)
    swim_on = built.kw["probe_interval"] > 0
    for v, c in built.cases.items():
        nd = Node(oracle, sim, v)
        row = rows[v]
        hot = set()
        for i, (_, _, _, (kind, key, val, flags)) in enumerate(c.arrivals):
            tg = {}
            if kind in (EVENT, QUERY):
                ring, clk = (er, int(row["event_clock"])) if kind == EVENT else (qr, int(row["query_clock"]))
                b = ring[1 + val % RING, v]
                keys = [int(x) for x in b["keys"]]
                cur = val + 1 if val >= clk else clk
                tg["ring.mintime"] = bool(row["flags"] & 16)
                tg["ring.old"] = cur > RING and ((kind == EVENT and val < cur - RING) or (kind == QUERY and RING < cur - RING))
                tg["ring.bucket_present"] = keys[0] != 0
                tg["ring.key_in_head"] = keys[0] != 0 and key in keys[:2]
                tg["ring.key_in_tail"] = key in keys[2:]
                tg["ring.second_key"] = keys[1] != 0
                tg["ring.adv"] = val >= clk
                if kind == QUERY and keys[0] != 0:
                    tg["ring.q2_same_time"] = int(b["ltime"]) == val
            elif key < n:
                try:
                    e = nd.view(key)
                except AssertionError:
                    e = None
                tg["member.has_slot"] = e is not None
                if kind in (JOIN, LEAVE):
                    tg["jl.adv"] = val >= int(row["clock"])
                if e is not None:
                    known = bool(e["known"])
                    tg["member.known"] = known
                    if kind in (JOIN, LEAVE):
                        tg["jl.lt_le_entry"] = val <= e["ltime"]
                        tg["jl.intent_buffered"] = (not known) and ((nd.recent_intent(key, 1) is not None) or (nd.recent_intent(key, 2) is not None))
                        tg["walk.trigger_prune"] = kind == LEAVE and bool(flags & PRUNE)
                    elif swim_on:
                        inc, frm = val & 0xFFFFFFFF, val >> 32
                        tg["swim.self"] = key == v
                        if kind == AL:
                            tg["alive.inc_le"] = inc <= (int(row["inc"]) if key == v else e["inc"])
                            tg["walk.trigger_alive"] = True
                        else:
                            tg["sd.inc_lt"] = inc < e["inc"]
                            tg["sd.gone"] = e["swim"] >= 2
                            tg["tail.inc_ge"] = inc >= e["inc"]
                            if kind == SUSPECT:
                                tg["walk.trigger_alive"] = False
                                tg["sd.fully_confirmed"] = e["swim"] == 1 and e["nconf"] >= kconf
                                tg["sd.suspected"] = e["swim"] == 1
                                if e["swim"] == 1:
                                    tg["tail.confirmer_counted"] = frm in e["conf"][:e["nconf"] + 1]
                                    tg["tail.stale_conf_word"] = frm in e["conf"][e["nconf"] + 1:]
                    tg["walk.subject_hot"] = (key & 15) in hot
                if kind == AL or (kind == LEAVE and flags & PRUNE):
                    hot.add(key & 15)
            for k, val_ in tg.items():
                c.tags.setdefault(k, set()).add(bool(val_))
            c.handled.append(not verdict(tg, kind, bool(row["flags"] & 1) and not c.state.get("down"), swim_on))


# ------------------------------------------------------------------------------------------------ the variants both test files run
ONE_PAGE = ("page", "packets")
VARIANTS = {
    # name: (what the table holds, build arguments)
    "bijection-p4": (dict(places=ONE_PAGE, floods=8), dict()),
    "bijection-p16": (dict(only=("pairs", "triples"), floods=4), dict(pkt_records=16)),
    "bijection-sharded": (dict(places=ONE_PAGE, floods=8), dict(vshards=4, chunks=2)),
    "random-dense": (dict(places=ONE_PAGE, floods=28), dict(random_fanout=True, n=3072)),
    "random-sparse": (dict(places=ONE_PAGE), dict(random_fanout=True, layout="sparse", n=10240)),
    "random-ragged": (dict(places=ONE_PAGE, only=("pairs", "triples")), dict(random_fanout=True, n=2049, ragged=True)),
    "random-p8": (dict(only=("pairs", "triples"), floods=4), dict(random_fanout=True, pkt_records=8, n=3072)),
    "random-small-0": (dict(only=("singles",), part=(0, 5)), dict(random_fanout=True, n=200)),
    "random-small-1": (dict(only=("singles",), part=(1, 5)), dict(random_fanout=True, n=200)),
    "random-small-2": (dict(only=("singles",), part=(2, 5)), dict(random_fanout=True, n=200)),
    "random-small-3": (dict(only=("singles",), part=(3, 5)), dict(random_fanout=True, n=200)),
    "random-small-4": (dict(only=("singles",), part=(4, 5)), dict(random_fanout=True, n=200)),
    "bijection-noswim": (dict(places=("page",)), dict(probe_interval=0)),
    "random-noswim": (dict(places=("page",)), dict(random_fanout=True, probe_interval=0, n=2560)),
}
_built = {}


def ragged_cases():
    """for the one node of a ragged cluster's last wave: the order-dependent pair of the issue's trial"""
    return [Case("pairs", "ragged/LEAVEp@14>JOIN@12", dict(member="alive", swim="alive", clock=20), [(LEAVE, "X", L + 2, PRUNE), (JOIN, "X", L, 0)], "packets")]


def built(oracle, name):
    """the variant's image, built once per session and shared read-only"""
    if name not in _built:
        tab, args = VARIANTS[name]
        args = dict(args)
        tab = dict(tab)
        part = tab.pop("part", None)
        probe = _ffi.Sim(oracle, _ffi.make_config(64, probe_interval=5 if args.get("probe_interval", 5) else 0, view_slots=VIEW_SLOTS))
        cases = table(kconf_of(oracle, probe) if args.get("probe_interval", 5) else 3, **tab)
        if part:
            cases = cases[part[0]::part[1]]
        last = ragged_cases() if args.pop("ragged", False) else ()
        n = args.pop("n", None) or (len(cases) + 64 + 63) // 64 * 64
        _built[name] = build(oracle, cases, n, last_wave=last, **args)
    return _built[name]


def verdict(tg, kind, up, swim_on):
    """True when the receive path retires the record WITHOUT a handler, from the record's tags: what the comments of fast_noop,
    fast_retire and tail_retire say they retire, judged against the state as the tick began — a duplicate, an old message, a subject
    without a view slot, nothing that advances a clock; on the second look a key in a bucket's tail, a counted confirmer.  Used to
    count the records the classification should leave for the handlers (a verdict that retires LESS changes no state: only this
    count shows it); never to decide what a record does."""
    if not up:
        return True
    if kind in (EVENT, QUERY):
        if tg["ring.adv"] or tg["ring.mintime"]:
            return False
        same = kind == EVENT or tg.get("ring.q2_same_time", False)
        if tg["ring.old"] or (tg["ring.bucket_present"] and same and tg["ring.key_in_head"]):
            return True
        return tg["ring.bucket_present"] and tg["ring.second_key"] and same and tg["ring.key_in_tail"]   # the second look needs a bucket with two keys and more
    if not tg.get("member.has_slot", False):
        return not tg.get("jl.adv", False) if kind in (JOIN, LEAVE) else True
    if kind in (JOIN, LEAVE):
        return tg["jl.lt_le_entry"] and (tg["member.known"] or tg["jl.intent_buffered"]) and not tg["jl.adv"]
    if not swim_on:
        return True
    if kind == AL:
        return tg["alive.inc_le"] and (tg["swim.self"] or tg["member.known"])
    if not tg["member.known"] or tg["sd.inc_lt"] or tg["sd.gone"] or (kind == SUSPECT and tg["sd.fully_confirmed"]):
        return True
    return kind == SUSPECT and tg["sd.suspected"] and tg["tail.confirmer_counted"]


def handled_by_kind(built):
    """{kind: records the classification leaves for the handlers} over every case of the cluster"""
    out = {k: 0 for k in KIND_NAME}
    for c in built.cases.values():
        for (_, _, _, rec), h in zip(c.arrivals, c.handled):
            out[rec[0]] += bool(h)
    return out
