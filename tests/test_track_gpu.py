"""Device-resident trackers (include/serf_sim_track.h) on the GPU: every field of every sim_track_result equals what the
reference model (tests/track_model.py) computes from the CPU oracle stepped one tick at a time.  The HIP handle is
driven in long sim_step calls and read once at the end; comparisons are exact."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests.track_model import FIELDS, TrackModel

pytestmark = pytest.mark.gpu

KW = dict(fanout=4, view_slots=64, event_ring=64, query_ring=64, probe_interval=5, loss=0.01, ring_overflow=4,
          push_pull_interval=150, join_sync=True)
KRANDOM = _ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT
BIJECTION = _ffi.CF_BASELINE_JOINED
FAILED = 1 << _ffi.STATUS_FAILED
SUSPECT_OR_DEAD = 1 << _ffi.SWIM_SUSPECT | 1 << _ffi.SWIM_DEAD


def script(n, seed=11):
    """6 crashes at ticks 10, 17, ..., 45; 6 nodes that never crash; 40 user events from tick 20 every 4 ticks."""
    rng = np.random.default_rng(seed)
    crashed = rng.choice(n, 6, replace=False).tolist()
    crash_at = [10 + 7 * i for i in range(6)]
    live = [x for x in rng.choice(n, 12, replace=False).tolist() if x not in crashed][:6]
    events = []
    for i in range(40):
        node = int(rng.integers(0, n))
        while node in crashed:
            node = int(rng.integers(0, n))
        events.append((20 + 4 * i, node, 0x40000000 + i))
    return dict(crashed=crashed, crash_at=crash_at, live=live, events=events)


def member_specs(s):
    out = []
    for t, c in zip(s["crash_at"], s["crashed"]):
        out.append(_ffi.member_tracker(c, FAILED, SUSPECT_OR_DEAD, start=t))   # "suspected or worse"
        out.append(_ffi.member_tracker(c, FAILED, start=t))                    # "declared failed"
    for c in s["live"]:
        out.append(_ffi.member_tracker(c, FAILED, SUSPECT_OR_DEAD))            # false positives
    return out


def drive(sim, s, ticks, add_many, step, track=True, on_stretch=None):
    """The same script for both sides: MEMBER trackers up front, one EVENT tracker per user event, registered with the
    Lamport time its origin is about to give it; the run advances in ONE step(k) per stretch between two injections."""
    for t, c in zip(s["crash_at"], s["crashed"]):
        sim.inject(t, _ffi.OP_CRASH, c)
    handles = list(add_many(member_specs(s))) if track else []
    for te, node, key in s["events"]:
        if te >= ticks:
            break
        step(te - sim.tick)
        if on_stretch:
            on_stretch()
        if track:
            handles += add_many([_ffi.rumour_tracker(_ffi.K_EVENT, key, sim.stats(node).event_time)])
        sim.user_event(node, key, 64)
    step(ticks - sim.tick)
    if on_stretch:
        on_stretch()
    return handles


def model_side(oracle, n, s, ticks, **kw):
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = TrackModel(o)
    hs = drive(o, s, ticks, lambda specs: [m.add(x) for x in specs], m.step)
    return o, m, [m.result(h) for h in hs]


def hip_side(n, s, ticks, **kw):
    g = serf_amd.create(n, **kw)
    ids = drive(g, s, ticks, g.track_add, g.step)
    return g, ids, [r.as_dict() for r in g.track_read(ids)]      # read once, at the end


def assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert set(a) == set(FIELDS) == set(b)
        assert a == b, f"{what}: tracker {i}: HIP {a} != model {b}"


def check_nontrivial(s, want):
    """The scenario does what it is for (otherwise equal results would show little)."""
    nv = len(s["crashed"])
    for i in range(nv):
        susp, failed = want[2 * i], want[2 * i + 1]
        assert susp["first"] != _ffi.TRACK_NEVER and failed["p99"] != _ffi.TRACK_NEVER, (susp, failed)
        assert s["crash_at"][i] < susp["first"] <= failed["first"] <= failed["p99"]
    ev = want[2 * nv + len(s["live"]):]
    assert ev and all(r["p99"] != _ffi.TRACK_NEVER for r in ev)


@pytest.mark.parametrize("variant", ["krandomnodes", "bijection", "pkt_records_16", "vshards_4"])
def test_parity_4096_nodes(oracle, hiplib, variant):
    n, ticks = 4096, 260
    kw = dict(KW, flags=BIJECTION if variant == "bijection" else KRANDOM)
    if variant == "pkt_records_16":
        kw["pkt_records"] = 16
    if variant == "vshards_4":
        kw["vshards"] = 4
    s = script(n)
    o, m, want = model_side(oracle, n, s, ticks, **kw)
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0      # the run stays inside the model's bounds
    g, ids, got = hip_side(n, s, ticks, **kw)
    assert_same(got, want, variant)
    assert len(got) == 12 + 6 + 40
    check_nontrivial(s, want)
    assert g.digest() == o.digest(), "trackers must not perturb the run"
    assert g.track_active() == (len(ids), sum(r["state"] != 2 for r in want))


def test_parity_at_size_65536_nodes_one_step_per_stretch(oracle, hiplib):
    n, ticks = 65536, 200
    kw = dict(KW, view_slots=16, flags=KRANDOM)
    s = script(n)
    o, m, want = model_side(oracle, n, s, ticks, **kw)
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    g, ids, got = hip_side(n, s, ticks, **kw)
    assert_same(got, want, "65536 nodes")
    nv = len(s["crashed"])
    assert all(want[2 * i]["first"] != _ffi.TRACK_NEVER for i in range(nv))
    assert any(want[2 * i + 1]["p99"] != _ffi.TRACK_NEVER for i in range(nv))
    assert g.digest() == o.digest()


def rumour_script(sim, add, step, remove=None):
    """LEAVE / JOIN / QUERY rumours; node 300 crashes, comes back and refutes, and once everybody holds it Alive again
    its view slot is recycled while trackers of it live (and new ones start on the baseline); windows that start in
    the future, in the past, and that run out; an id that is freed and reused."""
    hs = {}
    sim.inject(5, _ffi.OP_CRASH, 300)
    sim.inject(40, _ffi.OP_REVIVE, 300)
    step(3)
    hs["fail300"] = add(_ffi.member_tracker(300, FAILED, SUSPECT_OR_DEAD))
    hs["inc300"] = add(_ffi.member_tracker(300, 1 << _ffi.STATUS_ALIVE, min_inc=1))            # the refutation, seen by all
    hs["never300"] = add(_ffi.member_tracker(300, FAILED, SUSPECT_OR_DEAD, start=97))          # lives through the recycling pass
    hs["join300"] = add(_ffi.rumour_tracker(_ffi.K_JOIN, 300, 2))                              # likewise (nobody, ever)
    hs["leave100"] = add(_ffi.rumour_tracker(_ffi.K_LEAVE, 100, sim.stats(100).member_time))
    hs["left100"] = add(_ffi.member_tracker(100, 1 << _ffi.STATUS_LEFT | 1 << _ffi.STATUS_LEAVING))
    hs["future"] = add(_ffi.member_tracker(100, FAILED, start=40, max_age=25))                    # ticks 40 .. 64
    hs["aged"] = add(_ffi.member_tracker(100, 1 << _ffi.STATUS_LEFT, start=1, max_age=6))         # start in the past = now
    hs["short"] = add(_ffi.rumour_tracker(_ffi.K_LEAVE, 100, sim.stats(100).member_time, start=5, max_age=1))
    sim.leave(100)
    step(9)
    hs["leave2000"] = add(_ffi.rumour_tracker(_ffi.K_LEAVE, 2000, sim.stats(2000).member_time))
    hs["query"] = add(_ffi.rumour_tracker(_ffi.K_QUERY, 777, sim.stats(5).query_time))
    sim.leave(2000)
    sim.query(5, 777, _ffi.F_ACK)
    step(8)
    if remove:
        remove(hs.pop("aged"))            # retired long ago; its id is free again ...
    else:
        hs.pop("aged")
    hs["reused"] = add(_ffi.member_tracker(2000, 1 << _ffi.STATUS_LEFT, max_age=50))   # ... and goes to this one
    step(30)
    hs["join100"] = add(_ffi.rumour_tracker(_ffi.K_JOIN, 100, sim.stats(100).member_time))
    hs["rejoined"] = add(_ffi.member_tracker(100, 1 << _ffi.STATUS_ALIVE, min_inc=0, start=0, max_age=100))
    sim.join(100, 7)
    step(80)
    # tick 130: node 300 has no view slot any more; these read its baseline (Alive at incarnation 1)
    hs["base_inc1"] = add(_ffi.member_tracker(300, 1 << _ffi.STATUS_ALIVE, min_inc=1))
    hs["base_inc2"] = add(_ffi.member_tracker(300, 1 << _ffi.STATUS_ALIVE, min_inc=2))
    hs["base_join"] = add(_ffi.rumour_tracker(_ffi.K_JOIN, 300, 1))
    step(40)
    return hs


def test_rumours_recycled_slot_windows_and_id_reuse(oracle, hiplib):
    n = 4096
    kw = dict(fanout=4, view_slots=16, event_ring=64, query_ring=64, probe_interval=5, loss=0.01, push_pull_interval=150,
              join_sync=True, recycle_interval=20, flags=KRANDOM)
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = TrackModel(o)
    aged = {}

    def m_remove(h):
        aged["model"] = m.result(h)
        m.remove(h)
    mh = rumour_script(o, m.add, m.step, m_remove)
    cs = o.cluster_stats()
    assert cs["slots_recycled"] > 0 and 300 in m.base, "node 300's slot was to be recycled while its trackers live"
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0

    g = serf_amd.create(n, **kw)
    ids_seen = []

    def g_add(spec):
        ids_seen.append(g.track_add([spec])[0])
        return ids_seen[-1]

    def g_remove(i):
        aged["hip"] = g.track_read([i])[0].as_dict()
        aged["id"] = i
        g.track_remove([i])
        with pytest.raises(_ffi.SimError) as ei:
            g.track_read([i])
        assert ei.value.code == _ffi.EINVAL
    gh = rumour_script(g, g_add, g.step, g_remove)
    assert aged["hip"] == aged["model"] and aged["model"]["state"] == 2 and aged["model"]["evaluated"] == 6
    assert gh["reused"] == aged["id"], "a freed id is handed out again"
    names = sorted(mh)
    assert names == sorted(gh)
    got = [r.as_dict() for r in g.track_read([gh[k] for k in names])]
    want = [m.result(mh[k]) for k in names]
    assert_same(got, want, str(names))
    w = dict(zip(names, want))
    assert w["short"]["evaluated"] == 1 and w["short"]["state"] == 2
    assert w["future"]["evaluated"] == 25 and w["future"]["state"] == 2
    assert w["leave100"]["p99"] != _ffi.TRACK_NEVER and w["join100"]["p99"] != _ffi.TRACK_NEVER
    assert w["query"]["p99"] != _ffi.TRACK_NEVER and w["leave2000"]["all"] != _ffi.TRACK_NEVER
    assert w["base_inc1"]["all"] == 131 and w["base_inc2"]["peak"] == 0 and w["base_inc2"]["evaluated"] == 40
    assert w["base_join"]["all"] == 131 and w["join300"]["peak"] == 0 and w["join300"]["state"] == 1
    assert w["never300"]["evaluated"] == 170 - 97 and w["inc300"]["all"] != _ffi.TRACK_NEVER
    assert g.digest() == o.digest()


def many_specs(s, n):
    """SIM_TRACK_MAX trackers over 64 subjects (victims, nodes that stay up, others with and without a view slot)."""
    rng = np.random.default_rng(5)
    subjects = s["crashed"] + s["live"] + rng.choice(n, 52, replace=False).tolist()
    masks = [(FAILED, SUSPECT_OR_DEAD), (FAILED, 0), (1 << _ffi.STATUS_ALIVE, 0), (0, 1 << _ffi.SWIM_SUSPECT),
             (1 << _ffi.STATUS_NONE | 1 << _ffi.STATUS_LEFT, 1 << _ffi.SWIM_DEAD), (FAILED, 1 << _ffi.SWIM_ALIVE)]
    out = []
    for i in range(_ffi.TRACK_MAX):
        sm, wm = masks[(i // 64) % len(masks)]
        out.append(_ffi.member_tracker(subjects[i % 64], sm, wm, min_inc=(i // 384) % 2, start=i % 7 * 9, max_age=(0, 30, 100)[i % 3]))
    return out


def test_1024_trackers_at_once_and_errors(oracle, hiplib):
    n, ticks = 4096, 120
    kw = dict(KW, flags=KRANDOM)
    s = script(n)
    specs = many_specs(s, n)
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = TrackModel(o)
    g = serf_amd.create(n, **kw)
    for sim in (o, g):
        for t, c in zip(s["crash_at"], s["crashed"]):
            sim.inject(t, _ffi.OP_CRASH, c)
    mh = [m.add(x) for x in specs]
    ids = g.track_add(specs)
    assert sorted(ids) == list(range(_ffi.TRACK_MAX))
    # the 1025th: refused, nothing changes
    with pytest.raises(_ffi.SimError) as ei:
        g.track_add([_ffi.member_tracker(1, FAILED)])
    assert ei.value.code == _ffi.ERANGE
    assert g.track_active() == (_ffi.TRACK_MAX, _ffi.TRACK_MAX)
    bad = [_ffi.Tracker(0, 1, FAILED, 0, 0, 0, 0), _ffi.Tracker(3, 1, FAILED, 0, 0, 0, 0),
           _ffi.member_tracker(n, FAILED), _ffi.member_tracker(1, 0, 0), _ffi.member_tracker(1, 1 << 5),
           _ffi.member_tracker(1, FAILED, 1 << 4), _ffi.Tracker(_ffi.TRK_MEMBER, 1, FAILED, 0, 9, 0, 0),
           _ffi.rumour_tracker(_ffi.K_ALIVE, 1, 1), _ffi.rumour_tracker(_ffi.K_EVENT, 0, 1),
           _ffi.rumour_tracker(_ffi.K_JOIN, n, 1), _ffi.Tracker(_ffi.TRK_RUMOUR, _ffi.K_EVENT, 5, 1, 1, 0, 0)]
    g.track_remove(ids[-2:])          # room for the bad ones: they must fail for what they are
    for b in bad:
        with pytest.raises(_ffi.SimError) as ei:
            g.track_add([_ffi.member_tracker(2, FAILED), b])
        assert ei.value.code == _ffi.EINVAL, (b.kind, b.a, b.b)
    for call in (lambda: g.track_add([]), lambda: g.track_read([]), lambda: g.track_read([ids[-1]]),
                 lambda: g.track_remove([ids[-1]]), lambda: g.track_remove([ids[0], ids[0]]), lambda: g.track_read([_ffi.TRACK_MAX])):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.EINVAL
    assert g.track_active() == (_ffi.TRACK_MAX - 2, _ffi.TRACK_MAX - 2)
    assert g.track_add(specs[-2:]) == ids[-2:]          # freed ids are handed out again, lowest first
    g.step(ticks)
    m.step(ticks)
    got = [r.as_dict() for r in g.track_read(ids)]
    assert_same(got, [m.result(h) for h in mh], "1024 trackers")
    assert sum(r["peak"] > 0 for r in got) > 100 and sum(r["state"] == 2 for r in got) > 100
    assert g.digest() == o.digest()
    # a shard has no trackers; neither has a handle inside a tick
    sh = serf_amd.create(n, force_sharded=True, **kw)
    for call in (lambda: sh.track_add([_ffi.member_tracker(1, FAILED)]), lambda: sh.track_active()):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    t = serf_amd.create(256, fanout=3)
    t.step_begin()
    with pytest.raises(_ffi.SimError) as ei:
        t.track_add([_ffi.member_tracker(1, FAILED)])
    assert ei.value.code == _ffi.ESTATE
    t.close()


def test_trackers_do_not_interfere(hiplib):
    n, ticks = 4096, 260
    kw = dict(KW, flags=KRANDOM)
    s = script(n)
    runs = []
    for track in (False, True):
        g = serf_amd.create(n, **kw)
        watched = [s["live"][0], 3]
        for w in watched:
            g.watch(w)
        digests, evs = [], []

        def step(k, g=g, digests=digests, evs=evs):
            for _ in range(k):
                g.step(1)
                if g.tick % 8 == 0:
                    digests.append(g.digest())
                    evs.extend(g.drain_events())
        drive(g, s, ticks, g.track_add, step, track=track)
        evs.extend(g.drain_events())
        runs.append((digests, evs))
        if track:
            assert g.track_active()[0] == 58
        else:
            assert g.track_active() == (0, 0)
    assert len(runs[0][0]) == ticks // 8 and runs[0][0] == runs[1][0]
    assert runs[0][1] and runs[0][1] == runs[1][1]
