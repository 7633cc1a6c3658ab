"""Checkpoint / resume (sim_snapshot / sim_restore): the image is canonical, so a run can be stopped in one
implementation of the ABI and resumed in another — oracle -> oracle on CPU, oracle <-> HIP on the GPU box.
(Reference analogue: Snapshotter, serf-core/src/snapshot.rs:117-126,228-347, per node; here per simulation.)"""
import ctypes as C

import numpy as np
import pytest

from serf_amd import _ffi
from tests import _scenario as sc

KW = dict(fanout=3, view_slots=48, event_ring=16, query_ring=8, leave_delay=6, probe_interval=4, loss=0.03,
          push_pull_interval=5, reap_interval=9, reconnect_timeout=40, tombstone_timeout=60, intent_timeout=30)


def started(lib, n=384, ticks=45, **extra):
    kw = dict(KW, **extra)
    sim = _ffi.Sim(lib, _ffi.make_config(n, **kw))
    sc.apply_schedule(sim, sc.schedule(n, 80, rate=0.7, seed=21, max_member_subjects=40))   # part of it still pending at `ticks`
    sim.step(ticks)
    return sim, kw


def resume(lib, n, kw, image):
    sim = _ffi.Sim(lib, _ffi.make_config(n, **kw))
    sim.restore(image)
    return sim


def test_oracle_snapshot_resumes_identically(oracle):
    a, kw = started(oracle)
    img = a.snapshot()
    b = resume(oracle, 384, kw, img)
    assert b.tick == a.tick and b.digest() == a.digest()
    a.step(60)
    b.step(60)
    assert a.digest() == b.digest()
    sc.assert_same_state(a, b, "resumed oracle")
    assert a.stats(7).members == b.stats(7).members


def test_restore_rejects_wrong_config_and_used_handles(oracle):
    a, kw = started(oracle)
    img = a.snapshot()
    other = _ffi.Sim(oracle, _ffi.make_config(384, **dict(kw, fanout=4)))
    with pytest.raises(_ffi.SimError):
        other.restore(img)
    with pytest.raises(_ffi.SimError):
        a.restore(img)                       # a handle that has been stepped
    with pytest.raises(_ffi.SimError):
        resume(oracle, 384, kw, img[:100])   # truncated image


@pytest.mark.gpu
@pytest.mark.parametrize("vshards", [1, 4])
def test_oracle_image_resumes_on_hip_and_back(oracle, hiplib, vshards):
    a, kw = started(oracle, n=512, vshards=vshards)
    img = a.snapshot()
    g = resume(hiplib, 512, kw, img)
    assert g.tick == a.tick and g.digest() == a.digest()
    for t in range(6):
        a.step(10)
        g.step(10)
        assert a.digest() == g.digest(), f"diverged {10 * (t + 1)} ticks after the resume"
    sc.assert_same_state(g, a, "oracle image resumed on HIP")
    img2 = g.snapshot()                      # and back: HIP image into a fresh oracle
    b = resume(oracle, 512, kw, img2)
    assert b.digest() == g.digest()
    b.step(20)
    g.step(20)
    assert b.digest() == g.digest()
    assert np.array_equal(img2[:64], a.snapshot()[:64])   # same header for the same state


@pytest.mark.gpu
def test_huge_lamport_times_and_odd_ring_sizes(oracle, hiplib):
    # state no API call can reach quickly — Lamport clocks beyond 2^32, rings whose size is not a power
    # of two (64-bit modulo on the device), the query ring past quirk Q1's 2*B horizon — is built on the
    # oracle through its test hooks, carried over as a snapshot image, and must evolve identically on HIP
    from tests._oracle import Node
    n = 200
    kw = dict(KW, event_ring=12, query_ring=7, view_slots=40)
    a = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    for node, (c, e, q) in {3: (2 ** 33 + 5, 2 ** 34 + 1, 9), 77: (5, 2 ** 32 - 2, 2 ** 40), 150: (2 ** 63, 11, 13)}.items():
        nd = Node(oracle, a, node)
        nd.set_clock(Node.CLOCK, c)
        nd.set_clock(Node.EVENT, e)
        nd.set_clock(Node.QUERY, q)
    # EventCore / QueryCore min_time (snapshot restore, event_join_ignore: base.rs:146-147, delegate.rs:531-537)
    assert oracle.t["set_min_time"](a.h, 10, 1, 3) == 0
    assert oracle.t["set_min_time"](a.h, 11, 2, 2) == 0
    sc.apply_schedule(a, sc.schedule(n, 50, rate=1.0, seed=8, max_member_subjects=30))
    for t, node in ((1, 3), (2, 77), (3, 150), (4, 3)):
        a.inject(t, _ffi.OP_USER_EVENT, node, 9000 + t, 40)
        a.inject(t, _ffi.OP_QUERY, node, 9100 + t, _ffi.F_ACK)
    img = a.snapshot()
    g = resume(hiplib, n, kw, img)
    for t in range(8):
        a.step(10)
        g.step(10)
        assert a.digest() == g.digest(), f"diverged after {10 * (t + 1)} ticks"
    sc.assert_same_state(g, a, "huge clocks")
    assert a.dump(_ffi.ARR_ROWS)["event_clock"].max() > 2 ** 34


# ---- malformed images: sim_restore refuses them and leaves the handle the fresh one it was ----
# The image: header, then 16 x (u64 length, payload) in the order oracle/serf_oracle.c documents.
SECTIONS = ("rows", "queue", "inbox", "view", "ering", "qring", "slot_of", "subject_of", "base", "upmap", "qtab", "qbits",
            "ops", "alloc_tick", "qfilt", "tags")
HEADER = 8 + C.sizeof(_ffi.Config) + 8 + 8 + 16    # magic, abi | config | tick | n_slots, n_pending_ops | ops_dropped, slots_recycled
N_SLOTS_AT = 8 + C.sizeof(_ffi.Config) + 8
QF_WORDS = 16                                      # SIM_QF_WORDS: {query id, number of ids, tag mask, sealed, ids[12]}


def sections(img):
    """{name: (where its length word is, where its payload is, its length)}"""
    at, out = HEADER, {}
    for name in SECTIONS:
        n = int.from_bytes(img[at:at + 8].tobytes(), "little")
        out[name] = (at, at + 8, n)
        at += 8 + n
    assert at == img.size, "the walk over the sections ends where the image ends"
    return out


def words(img, sec, name):
    """a section as a copy of its u32 words"""
    _, at, n = sec[name]
    return np.frombuffer(img[at:at + n].tobytes(), "<u4").copy()


def patched(img, at, data):
    out = img.copy()
    out[at:at + len(data)] = np.frombuffer(bytes(data), np.uint8)
    return out


@pytest.fixture(scope="module")
def source(oracle):
    """(image at tick 45, its configuration, the digest at tick 45, the digest 20 ticks later): sparse view, SWIM on, part of
    the schedule still pending"""
    a, kw = started(oracle, n=384)
    img = a.snapshot()
    d0 = a.digest()
    a.step(20)
    return img, kw, d0, a.digest()


def truncated_and_mislabelled(img):
    at_len, _, n = sections(img)["view"]
    return [("cut to 100 bytes", img[:100]), ("cut by its last byte", img[:-1]),
            ("the view section's length word raised by 32", patched(img, at_len, (n + 32).to_bytes(8, "little")))]


def inconsistent(img, n=384):
    """images of the right shape whose content would index out of bounds on the device"""
    sec = sections(img)
    n_slots, n_pending = (int(x) for x in np.frombuffer(img[N_SLOTS_AT:N_SLOTS_AT + 8].tobytes(), "<u4"))
    assert n_pending > 0, "part of the schedule is still pending"
    slot_of, subject_of = words(img, sec, "slot_of"), words(img, sec, "subject_of")
    taken = np.flatnonzero(subject_of != 0xFFFFFFFF)
    assert taken.size >= 2 and n_slots >= 2, "slots have been handed out"
    subj = int(np.flatnonzero(slot_of != 0xFFFFFFFF)[0])
    a, b = int(taken[0]), int(taken[1])
    swapped = subject_of.copy()
    swapped[[a, b]] = swapped[[b, a]]
    return [("a slot_of entry set to n_slots", patched(img, sec["slot_of"][1] + 4 * subj, n_slots.to_bytes(4, "little"))),
            ("two subject_of entries swapped", patched(img, sec["subject_of"][1], swapped.tobytes())),
            ("the first pending operation's node set to N", patched(img, sec["ops"][1] + 12, n.to_bytes(4, "little"))),   # OpEnt: u64 tick, u32 op, u32 node, ...
            ("a tag-class byte set to 255", patched(img, sec["tags"][1] + 7, b"\xff")),
            ("a query filter's id count set to SIM_QF_IDS + 1", patched(img, sec["qfilt"][1] + 4 * (3 * QF_WORDS + 1), (_ffi.QF_IDS + 1).to_bytes(4, "little")))]


def refuses_all_then_restores(lib, source, cases):
    img, kw, d0, d20 = source
    fresh = _ffi.Sim(lib, _ffi.make_config(384, **kw))     # ONE handle throughout
    for what, bad in cases:
        with pytest.raises(_ffi.SimError) as ei:
            fresh.restore(bad)
        assert ei.value.code == _ffi.EINVAL, what
    fresh.restore(img)
    assert fresh.tick == 45 and fresh.digest() == d0, "a refused image left something behind"
    fresh.step(20)
    assert fresh.digest() == d20


def test_oracle_restore_refuses_malformed_images_and_stays_fresh(oracle, source):
    refuses_all_then_restores(oracle, source, truncated_and_mislabelled(source[0]))


@pytest.mark.gpu
def test_hip_restore_refuses_malformed_images_and_stays_fresh(hiplib, source):
    img = source[0]
    refuses_all_then_restores(hiplib, source, truncated_and_mislabelled(img) + inconsistent(img))
