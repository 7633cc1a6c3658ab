"""Known-answer tests of the reference replayed against the oracle's handlers.

Each test names the reference test it restates (paths under /root/reference/serf-core/src).  String
ids of the reference ("test", "foo", ...) become small integer node ids; node 0 plays `s1`.
These pin the oracle: tests/test_parity_gpu.py then pins the HIP path to the oracle.  The arms are also replayed ON THE GPU, through the
tick kernel's receive path: tests/delivery_table.py restates them as records in flight towards prepared nodes (its `kat/` cases, each
naming its test here), tests/test_delivery_table.py holds them to the literal answers, tests/test_delivery_table_gpu.py delivers them.
"""
import ctypes as C

import numpy as np
import pytest

from serf_amd import _ffi
from tests._oracle import Node

ALIVE, LEAVING, LEFT, FAILED, NONE = _ffi.STATUS_ALIVE, _ffi.STATUS_LEAVING, _ffi.STATUS_LEFT, _ffi.STATUS_FAILED, _ffi.STATUS_NONE
TEST, FOO, BAR, BAZ, TUBEZ = 1, 2, 3, 4, 5


def fresh(oracle, n=8, **kw):
    """A just-constructed Serf (Serf::new): only itself known, every clock at 1."""
    kw.setdefault("flags", 0)
    sim = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    return sim, Node(oracle, sim, 0)


def test_lamport_clock(oracle):
    # types/clock.rs:175-191 — a fresh LamportClock::new() is 0
    sim, s1 = fresh(oracle)
    s1.set_clock(Node.CLOCK, 0)
    assert s1.clock() == 0
    assert s1.increment() == 1
    assert s1.clock() == 1
    s1.witness(Node.CLOCK, 41)
    assert s1.clock() == 42
    s1.witness(Node.CLOCK, 41)
    assert s1.clock() == 42
    s1.witness(Node.CLOCK, 30)
    assert s1.clock() == 42


def test_initial_stats(oracle):
    # serf/base/tests/serf.rs:772-788 (serf_stats): member_time 1, event_time 1, 1 member, empty queues
    sim, s1 = fresh(oracle)
    st = sim.stats(0)
    assert (st.member_time, st.event_time, st.query_time) == (1, 1, 1)
    assert (st.members, st.failed, st.left) == (1, 0, 0)
    assert (st.intent_queue, st.event_queue, st.query_queue) == (0, 0, 0)
    assert st.health_score == 0


def test_recent_intent(oracle):
    # serf/base/tests/serf.rs:873-950 — `expire` stamps are 2 s (10 ticks) in the past
    sim, s1 = fresh(oracle)
    t = oracle.t
    now, past = 1000, 990
    assert s1.recent_intent(FOO, Node.JOIN) is None
    t["set_tick"](sim.h, past)
    assert s1.upsert_intent(FOO, Node.JOIN, 1)
    assert s1.upsert_intent(BAR, Node.LEAVE, 2)
    t["set_tick"](sim.h, now)
    assert s1.upsert_intent(BAZ, Node.JOIN, 3)
    t["set_tick"](sim.h, past)
    assert s1.upsert_intent(BAR, Node.JOIN, 4)
    assert not s1.upsert_intent(BAR, Node.JOIN, 0)
    assert s1.upsert_intent(BAR, Node.JOIN, 5)
    assert s1.recent_intent(FOO, Node.JOIN) == 1
    assert s1.recent_intent(BAR, Node.JOIN) == 5
    assert s1.recent_intent(BAZ, Node.JOIN) == 3
    assert s1.recent_intent(TUBEZ, Node.JOIN) is None
    big = 1 << 20
    s1.reap(now, big, big, 5)  # reap_intents(now, 1 s)
    assert s1.recent_intent(FOO, Node.JOIN) is None
    assert s1.recent_intent(BAR, Node.JOIN) is None
    assert s1.recent_intent(BAZ, Node.JOIN) == 3
    s1.reap(now + 10, big, big, 5)  # now + 2 s
    assert s1.recent_intent(BAZ, Node.JOIN) is None


def test_join_intent_buffer_early(oracle):
    # serf/base/tests/serf/join.rs:8-35
    sim, s1 = fresh(oracle)
    assert s1.join_intent(TEST, 10), "should rebroadcast"
    assert not s1.join_intent(TEST, 10), "should not rebroadcast"
    assert s1.recent_intent(TEST, Node.JOIN) == 10


def test_join_intent_old_message(oracle):
    # join.rs:38-85
    sim, s1 = fresh(oracle)
    s1.set_member(TEST, ALIVE, 12)
    assert not s1.join_intent(TEST, 10)
    assert s1.recent_intent(TEST, Node.JOIN) is None


def test_join_intent_newer(oracle):
    # join.rs:88-134
    sim, s1 = fresh(oracle)
    s1.set_member(TEST, ALIVE, 12)
    assert s1.join_intent(TEST, 14)
    assert s1.recent_intent(TEST, Node.JOIN) is None
    assert s1.member(TEST) == (ALIVE, 14)
    assert s1.clock() == 15


def test_join_intent_reset_leaving(oracle):
    # join.rs:137-185
    sim, s1 = fresh(oracle)
    s1.set_member(TEST, LEAVING, 12)
    assert s1.join_intent(TEST, 14)
    assert s1.member(TEST) == (ALIVE, 14)
    assert s1.clock() == 15


def test_join_pending_intent(oracle):
    # join.rs:267-302
    sim, s1 = fresh(oracle)
    s1.upsert_intent(TEST, Node.JOIN, 5)
    s1.notify_join(TEST)
    assert s1.member(TEST) == (ALIVE, 5)


def test_join_pending_intents(oracle):
    # join.rs:305-347
    sim, s1 = fresh(oracle)
    s1.upsert_intent(TEST, Node.JOIN, 5)
    s1.upsert_intent(TEST, Node.LEAVE, 6)
    s1.notify_join(TEST)
    assert s1.member(TEST) == (LEAVING, 6)


def test_leave_intent_buffer_early(oracle):
    # serf/base/tests/serf/leave.rs:4-33
    sim, s1 = fresh(oracle)
    assert s1.leave_intent(TEST, 10)
    assert not s1.leave_intent(TEST, 10)
    assert s1.recent_intent(TEST, Node.LEAVE) == 10


def test_leave_intent_old_message(oracle):
    # leave.rs:36-82
    sim, s1 = fresh(oracle)
    s1.set_member(TEST, ALIVE, 12)
    assert not s1.leave_intent(TEST, 10)
    assert s1.recent_intent(TEST, Node.LEAVE) is None


def test_leave_intent_newer(oracle):
    # leave.rs:85-136
    sim, s1 = fresh(oracle)
    s1.set_member(TEST, ALIVE, 12)
    assert s1.leave_intent(TEST, 14)
    assert s1.recent_intent(TEST, Node.LEAVE) is None
    assert s1.member(TEST) == (LEAVING, 14)
    assert s1.clock() == 15


def test_leave_intent_state_arms(oracle):
    # base.rs:1497-1569: status_time is always updated; Failed -> Left moves failed -> left list
    sim, s1 = fresh(oracle)
    s1.set_member(TEST, FAILED, 3)
    assert sim.stats(0).failed == 1
    assert s1.leave_intent(TEST, 9)
    assert s1.member(TEST) == (LEFT, 9)
    st = sim.stats(0)
    assert (st.failed, st.left) == (0, 1)
    assert not s1.leave_intent(TEST, 9)  # `<=` => no infinite rebroadcast (event.rs:348)
    assert s1.leave_intent(TEST, 10)     # Left stays Left, still rebroadcast (base.rs:1512)
    assert s1.member(TEST) == (LEFT, 10)
    s1.set_member(FOO, NONE, 1)
    assert not s1.leave_intent(FOO, 5)   # None arm returns false AFTER updating status_time (A.7)
    assert s1.member(FOO) == (NONE, 5)


def test_leave_intent_refute_self(oracle):
    # base.rs:1470-1480 + broadcast_join base.rs:381-397: an Alive node refutes a leave about itself
    sim, s1 = fresh(oracle)
    assert s1.member(0) == (ALIVE, 0)
    assert not s1.leave_intent(0, 7)
    # witness(7) -> clock 8; broadcast_join(ltime=8): witness -> 9, own status_time 8, join queued
    assert s1.clock() == 9
    assert s1.member(0) == (ALIVE, 8)
    assert sim.stats(0).intent_queue == 1
    assert not s1.leave_intent(0, 7)  # now stale
    assert sim.stats(0).intent_queue == 1


def test_prune(oracle):
    # base.rs:1502-1511,1628-1653: prune erases the member
    sim, s1 = fresh(oracle)
    s1.set_member(TEST, ALIVE, 2)
    assert sim.stats(0).members == 2
    assert s1.leave_intent(TEST, 5, prune=True)
    assert s1.member(TEST) == (NONE, 0)
    assert sim.stats(0).members == 1


def test_user_event_old_message(oracle):
    # serf/base/tests/serf/event.rs:8-31
    sim, s1 = fresh(oracle)
    s1.witness(Node.EVENT, 512 + 1000)
    assert not s1.user_event(0x01D, 1)


def test_user_event_same_clock(oracle):
    # event.rs:34-85: three distinct (name,payload) at ltime 1 all rebroadcast, duplicates do not
    sim, s1 = fresh(oracle)
    sim.watch(0)
    for key in (101, 102, 103):
        assert s1.user_event(key, 1)
    for key in (101, 102, 103):
        assert not s1.user_event(key, 1)
    ev = sim.drain_events()
    assert [(e[2], e[3]) for e in ev] == [(5, 101), (5, 102), (5, 103)]  # delivered in order


def test_user_event_quirk_u1(oracle):
    # base.rs:801-807: an existing bucket's ltime is not compared
    sim, s1 = fresh(oracle, event_ring=8)
    assert s1.user_event(7, 3)
    assert not s1.user_event(7, 3 + 8)  # same key one ring-lap later is treated as a duplicate
    assert s1.user_event(9, 3 + 8)


def test_query_old_message(oracle):
    # event.rs:638-671 (passes through quirk Q1, base.rs:1012-1014)
    sim, s1 = fresh(oracle)
    s1.witness(Node.QUERY, 512 + 1000)
    assert not s1.query(1, 1)


def test_query_same_clock(oracle):
    # event.rs:674-772
    sim, s1 = fresh(oracle)
    for qid in (1, 2, 3):
        assert s1.query(qid, 1)
        assert not s1.query(qid, 1)
    assert s1.clock(Node.QUERY) == 2
    assert not s1.query(4, 1, flags=_ffi.F_NO_BROADCAST)  # base.rs:1062-1066


def test_query_quirks(oracle):
    # Q1: once query_clock > 2*B every query is dropped; Q2: bucket ltime never updated
    sim, s1 = fresh(oracle, query_ring=8)
    assert s1.query(5, 2)
    assert s1.query(5, 10)        # different ltime, same bucket: pushed, bucket.ltime stays 2
    assert s1.query(5, 10)        # ... so the repeat is NOT recognised (Q2)
    s1.witness(Node.QUERY, 17)
    assert not s1.query(6, 17)    # Q1: 8 < 18 - 8


def test_merge_remote_state(oracle):
    # serf/base/tests/serf/delegate.rs:117-180
    sim, s1 = fresh(oracle)
    subj = (C.c_uint32 * 2)(TEST, FOO)
    stl = (C.c_uint64 * 2)(20, 15)
    left = (C.c_uint32 * 1)(FOO)
    evl = (C.c_uint64 * 1)(45)
    evk = (C.c_uint32 * 1)(777)
    rc = oracle.t["merge_remote_state"](sim.h, 0, 42, 50, 100, subj, stl, 2, left, 1, evl, evk, 1, 0, 0)
    assert rc == 0
    assert s1.clock() == 42
    assert s1.recent_intent(TEST, Node.JOIN) == 20
    assert s1.recent_intent(FOO, Node.LEAVE) == 16
    assert s1.clock(Node.EVENT) == 50
    ring = sim.dump(_ffi.ARR_ERING).reshape(512, 8)
    assert ring[45, 0]["keys"][0] == 777 and ring[45, 0]["ltime"] == 45
    assert s1.clock(Node.QUERY) == 100


def test_queue_max(oracle):
    # serf/base/tests/serf.rs:57-160 (serf_get_queue_max)
    qm = oracle.t["queue_max"]
    assert qm(100, 4096, 0) == 4096
    assert qm(100, 4096, 1024) == 1024
    assert qm(100, 4096, 16) == 200
    assert qm(101, 4096, 16) == 202


def test_notify_leave_and_rejoin(oracle):
    # base.rs:1375-1440 + 1234-1274,1317-1320; event sequence of event.rs:118-129 (Join, Failed)
    sim, s1 = fresh(oracle)
    sim.watch(0)
    s1.notify_join(TEST)
    assert s1.member(TEST) == (ALIVE, 0)
    s1.notify_leave(TEST)
    assert s1.member(TEST)[0] == FAILED
    assert sim.stats(0).failed == 1
    s1.notify_leave(TEST)  # bad state, ignored
    assert sim.stats(0).failed == 1
    s1.notify_join(TEST)
    assert s1.member(TEST) == (ALIVE, 0)  # status_time kept
    assert sim.stats(0).failed == 0
    s1.leave_intent(TEST, 4)
    s1.notify_leave(TEST)
    assert s1.member(TEST) == (LEFT, 4)
    assert sim.stats(0).left == 1
    types = [e[2] for e in sim.drain_events()]
    assert types == [0, 2, 0, 1]  # Join, Failed, Join, Leave


def test_reaper(oracle):
    # serf/base/tests/serf/reap.rs:41-129: tombstone 6 s = 30 ticks, intent timeout 7 s = 35 ticks
    sim, s1 = fresh(oracle, n=16)
    now = 500
    s1.set_member(10, LEFT, 0, stamp=now)
    s1.set_member(11, LEFT, 0, stamp=now - 25)
    s1.set_member(12, LEFT, 0, stamp=now - 50)
    alice, bob, carol, doug = 5, 6, 7, 8
    t = oracle.t
    t["set_tick"](sim.h, now); s1.upsert_intent(alice, Node.JOIN, 1)
    t["set_tick"](sim.h, now - 50); s1.upsert_intent(bob, Node.JOIN, 2)
    t["set_tick"](sim.h, now); s1.upsert_intent(carol, Node.LEAVE, 1)
    t["set_tick"](sim.h, now - 50); s1.upsert_intent(doug, Node.LEAVE, 2)
    t["set_tick"](sim.h, now)
    assert sim.stats(0).left == 3
    s1.reap(now, 1 << 20, 30, 35)
    assert sim.stats(0).left == 2
    assert s1.recent_intent(alice, Node.JOIN) == 1
    assert s1.recent_intent(bob, Node.JOIN) is None
    assert s1.recent_intent(carol, Node.LEAVE) == 1
    assert s1.recent_intent(doug, Node.LEAVE) is None


def test_remove_old_member(oracle):
    # serf/base/tests/serf/remove.rs:187-222 — 3 entries, removing one id leaves 2
    sim, s1 = fresh(oracle)
    for s in (TEST, FOO, BAR):
        s1.set_member(s, LEFT, 1)
    assert sim.stats(0).left == 3
    s1.notify_join(FOO)  # base.rs:1317-1320 -> remove_old_member
    assert sim.stats(0).left == 2
