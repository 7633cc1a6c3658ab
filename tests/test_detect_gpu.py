"""Detection log (include/serf_sim_detect.h) on the GPU: every word of every header, every log record and every open episode
equals what the reference model (tests/detect_model.py) folds from the census records of the CPU oracle stepped one tick at a
time.  The HIP handle is driven in one sim_step per stretch between two injections and read once at the end; comparisons are
exact, and the digest at the end equals the oracle's: a detection log must not perturb the run."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_track_gpu as tt
from tests.census_model import CensusModel
from tests._oracle import load_oracle
from tests.detect_model import DetectModel
from tests.roll_model import RollModel
from tests.test_census import MAX_SUBJECTS, census_drive, census_kw
from tests.test_census_gpu import assert_same as census_same
from tests.test_detect import N, TICKS, check_consistent, oracle_run
from tests.test_roll_gpu import assert_same as roll_same
from tests.test_series import scenario

pytestmark = pytest.mark.gpu
NEVER = _ffi.DETECT_NEVER
DOWN, ACCUSED = _ffi.DETECT_DOWN, _ffi.DETECT_ACCUSED


def words(a, per):
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(a)))
    return a.view(np.uint64).reshape(len(a), per)


def same_words(got, want, per, what, names):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.shape}, the model has {want.shape}"
    g, w = words(got, per), words(want, per)
    bad = np.argwhere(g != w)
    msg = [f"{what} {i} word {j} ({names(j)}): HIP {int(g[i, j])} != model {int(w[i, j])}" for i, j in bad[:12].tolist()]
    assert not len(bad), f"{what}: {len(bad)} words differ\n" + "\n".join(msg)


def assert_same(g, want, what):
    """g: the HIP handle; want: (headers, log, open episodes) of the model.  Everything is read here, once."""
    wh, wl, wo = want
    same_words(g.detect_read(), wh, _ffi.DETECT_WORDS, f"{what}: header of sample", lambda j: f"tick word of the header's table: {j}")
    same_words(g.detect_log(), wl, _ffi.DETECT_EPISODE_WORDS, f"{what}: log record", lambda j: "episode word")
    same_words(g.detect_open(), wo, _ffi.DETECT_EPISODE_WORDS, f"{what}: open episode", lambda j: "episode word")


def model_of(m):
    return m.read(), m.log(), m.open()


def hip_run(variant, n, ticks, first=0, period=1, capacity=None, log_capacity=1 << 16, **over):
    g = serf_amd.create(n, **dict(census_kw(variant), **over))
    g.detect_start(first, period, capacity or ticks, log_capacity)
    census_drive(g, scenario(n), ticks, g.step)
    return g


@pytest.mark.parametrize("variant", ["krandomnodes", "lossy"])
def test_parity_4096_nodes_every_tick(hiplib, variant):
    o, m, wh, wl, wo = oracle_run(variant)
    g = hip_run(variant, N, TICKS)                 # driven in stretches
    assert g.detect_count() == m.count() == (TICKS, 0) and g.detect_log_count() == m.log_count()
    assert_same(g, (wh, wl, wo), variant)          # read once, at the end
    assert g.digest() == o.digest(), "a detection log must not perturb the run"
    # parts of the buffers
    same_words(g.detect_read(10, 5), wh[10:15], _ffi.DETECT_WORDS, variant + " headers [10, 15)", str)
    same_words(g.detect_read(TICKS - 1, 1), wh[-1:], _ffi.DETECT_WORDS, variant + " the last header", str)
    assert len(g.detect_read(TICKS, 0)) == 0
    same_words(g.detect_log(2, 3), wl[2:5], _ffi.DETECT_EPISODE_WORDS, variant + " log [2, 5)", str)
    same_words(g.detect_log(len(wl) - 1, 1), wl[-1:], _ffi.DETECT_EPISODE_WORDS, variant + " the last record", str)
    assert len(g.detect_log(len(wl), 0)) == 0
    check_consistent(g.detect_read(), g.detect_log(), g.detect_open())


def small_case(oracle, n, ticks, kw, script, **start):
    """script(sim, step) on the oracle with the model and on the HIP library; returns (handle, oracle, model)."""
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = DetectModel(o)
    m.start(0, 1, ticks, **start)
    script(o, m.step)
    g = serf_amd.create(n, **kw)
    g.detect_start(0, 1, ticks, **start)
    script(g, g.step)
    assert g.detect_count() == m.count() and g.detect_log_count() == m.log_count()
    return g, o, m


def test_eight_nodes(oracle, hiplib):
    """8 nodes, dense (8 slots): one partial wave of the kernel's one chunk."""
    n, ticks = 8, 60
    kw = dict(fanout=3, event_ring=64, query_ring=64, probe_interval=2)

    def run(sim, step):
        sim.inject(3, _ffi.OP_CRASH, 6)
        sim.inject(30, _ffi.OP_REVIVE, 6)
        step(5)
        sim.leave(2)
        step(ticks - 5)
    g, o, m = small_case(oracle, n, ticks, kw, run)
    wh, wl, wo = model_of(m)
    print("8 nodes: closed by outcome", wh["closed"][-1].tolist(), "open", len(wo))
    assert (wh["subjects"] == n).all() and int(wh["opened_down"][-1]) >= 1 and len(wl) >= 1
    assert_same(g, (wh, wl, wo), "8 nodes")
    assert g.digest() == o.digest()


def test_300_nodes_dense_two_returns_across_the_chunk_boundary(oracle, hiplib):
    """view_slots = 0: 300 slots, slot == id — a full chunk of 256 lanes and a partial one.  Ids 100 and 280 crash at one tick
    and are revived at one later tick: the two RETURNED records of one sample come from two chunks, in slot order."""
    n, ticks = 300, 60
    kw = dict(fanout=3, probe_interval=5, loss=0.02, event_ring=64, query_ring=64)

    def run(sim, step):
        for c in (100, 280):
            sim.inject(4, _ffi.OP_CRASH, c)
            sim.inject(20, _ffi.OP_REVIVE, c)
        step(ticks)
    g, o, m = small_case(oracle, n, ticks, kw, run)
    wh, wl, wo = model_of(m)
    ret = wl[wl["outcome"] == _ffi.DETECT_RETURNED]
    assert ret["slot"].tolist() == [100, 280] and ret["subject"].tolist() == [100, 280] and ret["closed"].tolist() == [21, 21]
    i = int(np.nonzero(wl["outcome"] == _ffi.DETECT_RETURNED)[0][0])
    assert wl["outcome"][i:i + 2].tolist() == [_ffi.DETECT_RETURNED] * 2 and int(wh["closed_now"][20]) >= 2
    assert (wh["subjects"] == n).all()
    assert_same(g, (wh, wl, wo), "300 nodes dense")
    assert g.digest() == o.digest()


def test_a_log_started_at_tick_60_opens_censored_episodes(hiplib):
    """The six crashed nodes are down when the log starts: their episodes are CENSORED — `opened` is the first sample, not
    the stop — and stay out of the latency histograms, though they are DETECTED and counted."""
    first = 60
    o, m, wh, wl, wo = oracle_run("krandomnodes", first=first)
    s = scenario(N)
    cens = wl[(wl["flags"] & _ffi.DETECT_F_CENSORED) != 0]
    assert sorted(cens["subject"].tolist()) == sorted(s["crashed"]) and (cens["opened"] == first + 1).all()
    assert (cens["outcome"] == _ffi.DETECT_DETECTED).all() and int(wh["closed"][-1][0]) == 6
    assert int(wh["hist_suspect"][-1].sum()) == 0 and int(wh["hist_all"][-1].sum()) == 0 and int(wh["hist_cleared"][-1].sum()) >= 1
    assert int(wh["open_down"][0]) == 6 and int(wh["tick"][0]) == first + 1 and m.count() == (TICKS - first, 0)
    g = serf_amd.create(N, **census_kw("krandomnodes"))

    def step(k):                                   # the log is started when the run has reached tick 60
        if g.tick < first < g.tick + k:
            k -= first - g.tick
            g.step(first - g.tick)
        if g.tick == first and g.detect_count() == (0, 0):
            g.detect_start(0, 1, TICKS, 1 << 16)   # (a first tick that has passed: now)
        g.step(k)
    census_drive(g, scenario(N), TICKS, step)
    assert g.detect_count() == m.count()
    assert_same(g, (wh, wl, wo), "started at tick 60")
    assert g.digest() == o.digest()


def test_period_3_and_a_buffer_smaller_than_the_run(hiplib):
    """first_tick 60 given at tick 0, a sample every third tick, room for 30 of the 47 that are due: the rest is dropped —
    evaluations not made; the episodes go on with the samples that are taken."""
    first, period, cap = 60, 3, 30
    due = len(range(first, TICKS, period))
    o = _ffi.Sim(load_oracle(), _ffi.make_config(N, **census_kw("lossy")))
    m = DetectModel(o)
    m.start(first, period, cap, 1 << 16)           # given at tick 0: the first sample is behind tick 60
    census_drive(o, scenario(N), TICKS, m.step)
    assert m.count() == (cap, due - cap) and due - cap > 0
    wh, wl, wo = model_of(m)
    assert wh["tick"].tolist() == [t + 1 for t in range(first, TICKS, period)][:cap]
    assert int(wh["closed"][-1].sum()) >= 6 and (wl["flags"] & _ffi.DETECT_F_CENSORED).any()
    g = hip_run("lossy", N, TICKS, first, period, cap)
    assert g.detect_count() == m.count()
    assert_same(g, (wh, wl, wo), "period 3, 30 samples")
    assert g.digest() == o.digest()


def test_a_log_of_three_records_keeps_the_first_three(hiplib):
    o, m, wh, wl, wo = oracle_run("krandomnodes", log_capacity=3)
    _, _, fh, fl, fo = oracle_run("krandomnodes")
    assert m.log_count() == (3, len(fl) - 3) and len(fl) >= 8
    same_words(wl, fl[:3], _ffi.DETECT_EPISODE_WORDS, "the model's own prefix", str)
    assert (wh["log_written"] == np.minimum(fh["log_written"], 3)).all() and (wh["log_lost"] == fh["log_written"] - wh["log_written"]).all()
    for f in ("closed", "false_declared", "opened_down", "hist_suspect", "hist_all", "hist_cleared", "closed_now"):
        assert (wh[f] == fh[f]).all(), f                # counters and histograms go on
    g = hip_run("krandomnodes", N, TICKS, log_capacity=3)
    assert g.detect_log_count() == (3, len(fl) - 3)
    assert_same(g, (wh, wl, wo), "log_capacity 3")
    with pytest.raises(_ffi.SimError) as ei:
        g.detect_log(3, 1)                               # beyond what was written
    assert ei.value.code == _ffi.EINVAL
    check_consistent(g.detect_read(), g.detect_log(), g.detect_open(), lost=len(fl) - 3)
    assert g.digest() == o.digest()


def test_slots_that_span_segments_65536_nodes(hiplib):
    """65 536 nodes, 16 view slots, a sample every 5 ticks: the census kernels in front of the log fold 8 segments a slot."""
    n, ticks = 65536, 120
    over = (("view_slots", 16),)
    o, m, wh, wl, wo = oracle_run("krandomnodes", n, ticks, 0, 5, 1000, 1 << 16, over)
    cs = o.cluster_stats()
    assert cs["overflow"] == 0 and cs["ops_dropped"] == 0
    assert int(wh["opened_down"][-1]) >= 6 and int(wh["subjects"].max()) >= 8 and len(wl) + len(wo) >= 6
    g = hip_run("krandomnodes", n, ticks, 0, 5, 1000, **dict(over))
    assert g.detect_count() == m.count() == (ticks // 5, 0)
    assert_same(g, (wh, wl, wo), "65536 nodes")
    assert g.digest() == o.digest()


def resume_drive(sim, s, resumed_at, ticks, step):
    """The rest of tests/test_series.drive on a handle that holds the state of tick `resumed_at` (the image brings the
    injected operations that are still pending with it)."""
    assert sim.tick == resumed_at
    for t, what, node, arg in s["actions"]:
        if t < resumed_at or t >= ticks:
            continue
        if t > sim.tick:
            step(t - sim.tick)
        if what == "event":
            sim.user_event(node, arg, 64)
        elif what == "leave":
            sim.leave(node)
        else:
            sim.query(node, arg, _ffi.F_ACK)
    step(ticks - sim.tick)


def test_a_running_log_across_sim_restore(oracle, hiplib):
    """sim_restore takes a handle at tick 0 only (SIM_ESTATE otherwise, on the oracle too): a log cannot have judged a sample
    before a restore, so no episode of its own can be open across one.  What a restore can do to a running log: the log is
    started on the fresh handle, sim_restore then jumps to tick 64 of the scenario, where six subjects are down already — the
    log is left as it is, its first sample is the one behind tick 64 and opens their episodes CENSORED.  The model is fed the
    same sequence of states: an oracle that makes the same jump."""
    T, ticks = 64, 150
    kw = census_kw("krandomnodes")
    s = scenario(N)
    src = _ffi.Sim(oracle, _ffi.make_config(N, **kw))
    census_drive(src, s, T, src.step)
    img = src.snapshot()
    o = _ffi.Sim(oracle, _ffi.make_config(N, **kw))
    m = DetectModel(o)
    m.start(0, 1, ticks, 1 << 10)
    o.restore(img)
    resume_drive(o, s, T, ticks, m.step)
    wh, wl, wo = model_of(m)
    assert m.count() == (ticks - T, 0) and int(wh["tick"][0]) == T + 1 and int(wh["open_down"][0]) == 6
    assert int(wh["closed"][-1][0]) == 6 and int((wl["flags"] & _ffi.DETECT_F_CENSORED).astype(bool).sum()) == 6 and int(wh["hist_all"][-1].sum()) == 0
    assert int(wh["closed"][-1][1]) == 1 and int(wh["closed"][-1][2]) >= 1          # the early crash and return: after the restore, from the image's pending operations
    g = serf_amd.create(N, **kw)
    g.detect_start(0, 1, ticks, 1 << 10)
    g.restore(img)
    assert g.tick == T and g.detect_count() == (0, 0)
    resume_drive(g, s, T, ticks, g.step)
    assert g.detect_count() == m.count()
    assert_same(g, (wh, wl, wo), "across a restore")
    assert g.digest() == o.digest()


def test_slots_recycled_between_two_samples_abandon_their_episodes(hiplib):
    """The lossy run sampled every 20 ticks — the period of its recycling pass: accusations of bystanders last about 14
    ticks, so a slot that held an accused subject at one sample is free, or another subject's, at the next: ABANDONED, the
    only outcome the other cases never reach.  The early crash returns between two samples and its slot has gone to
    somebody else by then: a DOWN episode is abandoned too."""
    period = 20
    o, m, wh, wl, wo = oracle_run("lossy", N, TICKS, 0, period, 1000)
    ab = wl[wl["outcome"] == _ffi.DETECT_ABANDONED]
    print("period 20: closed by outcome", wh["closed"][-1].tolist(), "abandoned", [(int(e["subject"]), int(e["slot"]), int(e["kind"])) for e in ab])
    assert m.count() == (TICKS // period, 0) and int(wh["closed"][-1][_ffi.DETECT_ABANDONED - 1]) == len(ab) >= 3
    assert (ab["kind"] == DOWN).any() and (ab["kind"] == ACCUSED).any()
    every = np.concatenate([wl, wo])
    taken_over = [e for e in ab if ((every["slot"] == e["slot"]) & (every["opened"] == e["closed"]) & (every["subject"] != e["subject"])).any()]
    assert taken_over, "no slot whose next subject opens an episode in the evaluation that abandons the last one's"
    g = hip_run("lossy", N, TICKS, 0, period, 1000)
    assert g.detect_count() == m.count()
    assert_same(g, (wh, wl, wo), "period 20")
    assert g.digest() == o.digest()


def test_census_roll_and_detection_log_on_one_handle(oracle, hiplib):
    """The three run together on one handle; each equals its result when it runs alone (its own model, which does not know
    the others — and for the log the handle of the parity test's configuration that ran it alone)."""
    n, ticks = N, 120
    kw = census_kw("lossy")
    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    cm, dm = CensusModel(o), DetectModel(o)
    rm = RollModel(o, lambda: (cm.after_tick(o.tick - 1), dm.after_tick(o.tick - 1)))
    rm.start(0, 2, ticks, 8, _ffi.ROLL_BY_ACCUSED)
    cm.start(0, 3, ticks, MAX_SUBJECTS)
    dm.start(0, 1, ticks, 1 << 10)
    census_drive(o, scenario(n), ticks, rm.step)
    g = serf_amd.create(n, **kw)
    g.roll_start(0, 2, ticks, 8, _ffi.ROLL_BY_ACCUSED)
    g.census_start(0, 3, ticks, MAX_SUBJECTS)
    g.detect_start(0, 1, ticks, 1 << 10)
    census_drive(g, scenario(n), ticks, g.step)
    assert g.detect_count() == dm.count() == (ticks, 0) and g.census_count() == cm.count() and g.roll_count() == rm.count()
    assert_same(g, model_of(dm), "a log next to a census and a roll")
    census_same(g.census_read(), cm.read(), "a census next to a log and a roll")
    roll_same(g.roll_read(), rm.read(), "a roll next to a census and a log")
    alone = serf_amd.create(n, **kw)
    alone.detect_start(0, 1, ticks, 1 << 10)
    census_drive(alone, scenario(n), ticks, alone.step)
    same_words(g.detect_read(), alone.detect_read(), _ffi.DETECT_WORDS, "together against alone: header", str)
    same_words(g.detect_log(), alone.detect_log(), _ffi.DETECT_EPISODE_WORDS, "together against alone: log", str)
    assert len(g.detect_log()) >= 3
    assert g.digest() == o.digest() == alone.digest()


def test_start_stop_start(oracle, hiplib):
    """The second log starts empty: no record, no open episode, no counter of the first."""
    n = 4096
    kw = census_kw("krandomnodes")

    def run(sim, det, step):
        sim.inject(2, _ffi.OP_CRASH, 500)
        sim.inject(14, _ffi.OP_REVIVE, 500)
        det.start(0, 1, 100, 16)
        step(20)
        first = det.snapshot()
        det.stop()
        det.start(0, 2, 100, 16)
        sim.inject(24, _ffi.OP_CRASH, 600)
        step(12)
        return first

    class Hip:
        def __init__(self, g):
            self.g, self.start, self.stop = g, g.detect_start, g.detect_stop

        def snapshot(self):
            return self.g.detect_read(), self.g.detect_log(), self.g.detect_open()

    o = _ffi.Sim(oracle, _ffi.make_config(n, **kw))
    m = DetectModel(o)
    m.snapshot = lambda: model_of(m)
    want1 = run(o, m, m.step)
    g = serf_amd.create(n, **kw)
    got1 = run(g, Hip(g), g.step)
    assert len(want1[1]) >= 1 and int(want1[0]["opened_down"][-1]) == 1
    for a, b, per, what in zip(got1, want1, (64, 8, 8), ("header", "log record", "open episode")):
        same_words(a, b, per, "the first log: " + what, str)
    wh, wl, wo = model_of(m)
    assert m.count() == (6, 0) and wh["tick"].tolist() == [21, 23, 25, 27, 29, 31] and int(wh["opened_down"][-1]) == 1
    assert int(wh["closed"][0].sum()) + int(wh["log_written"][0]) <= int(wh["closed_now"][0])        # nothing of the first log
    assert g.detect_count() == (6, 0)
    assert_same(g, (wh, wl, wo), "the second log")
    g.detect_stop()
    assert g.detect_count() == (0, 0) and g.detect_log_count() == (0, 0)
    assert g.digest() == o.digest()


def test_errors_leave_everything_as_it_was(hiplib):
    n = 4096
    kw = census_kw("krandomnodes")
    sh = serf_amd.create(n, force_sharded=True, **kw)      # a shard has no detection log
    for call in (lambda: sh.detect_start(0, 1, 8, 4), sh.detect_count, lambda: sh.detect_read(0, 0), sh.detect_log_count,
                 lambda: sh.detect_log(0, 0), sh.detect_open, sh.detect_stop):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    g = serf_amd.create(n, **kw)
    assert g.detect_count() == (0, 0) and g.detect_log_count() == (0, 0)
    for call in (lambda: g.detect_read(0, 0), lambda: g.detect_log(0, 0), g.detect_open, g.detect_stop):    # no log yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    for args in ((0, 0, 8, 4), (0, 1, 0, 4), (0, 1, _ffi.DETECT_MAX_SAMPLES + 1, 4), (0, 1, 8, 0), (0, 1, 8, _ffi.DETECT_MAX_LOG + 1)):
        with pytest.raises(_ffi.SimError) as ei:
            g.detect_start(*args)
        assert ei.value.code == _ffi.EINVAL and g.detect_count() == (0, 0)
    g.inject(1, _ffi.OP_CRASH, 9)
    g.detect_start(0, 1, 8, 4)
    g.step(3)
    assert g.detect_count() == (3, 0)
    before = g.detect_read(), g.detect_log(), g.detect_open()
    assert before[0]["open_down"].tolist() == [0, 1, 1] and len(before[1]) == 0 and before[2]["subject"].tolist() == [9]
    with pytest.raises(_ffi.SimError) as ei:
        g.detect_start(0, 1, 8, 4)                         # one log at a time
    assert ei.value.code == _ffi.ESTATE
    with pytest.raises(_ffi.SimError) as ei:
        g.detect_start(0, 0, 8, 4)                         # bad arguments come first
    assert ei.value.code == _ffi.EINVAL
    for first, cnt in ((0, 4), (3, 1), (4, 0)):            # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.detect_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL
    for first, cnt in ((0, 1), (1, 0)):                    # beyond `written`
        with pytest.raises(_ffi.SimError) as ei:
            g.detect_log(first, cnt)
        assert ei.value.code == _ffi.EINVAL
    C = _ffi.C
    fn, out, got = g.lib.f["detect_read"], np.zeros(2 * 64, np.uint64), C.c_uint32(77)
    assert fn(g.h, 0, 3, out.ctypes.data, out.size, C.byref(got)) == _ffi.EINVAL                  # a buffer one sample short
    assert fn(g.h, 0, 2, None, out.size, C.byref(got)) == _ffi.EINVAL and fn(g.h, 0, 2, out.ctypes.data, out.size, None) == _ffi.EINVAL
    fn, ep = g.lib.f["detect_log_read"], np.zeros(2, _ffi.DETECT_EPISODE_DTYPE)
    assert fn(g.h, 0, 0, None, 0, C.byref(got)) == _ffi.EINVAL and fn(g.h, 0, 0, ep.ctypes.data, 2, None) == _ffi.EINVAL
    fn = g.lib.f["detect_open"]
    assert fn(g.h, ep.ctypes.data, 0, C.byref(got)) == _ffi.EINVAL                                # one open episode, room for none
    assert fn(g.h, None, 2, C.byref(got)) == _ffi.EINVAL and fn(g.h, ep.ctypes.data, 2, None) == _ffi.EINVAL
    fn = g.lib.f["detect_log_count"]
    w = C.c_uint64(5)
    assert fn(g.h, None, C.byref(w)) == _ffi.EINVAL and fn(g.h, C.byref(w), None) == _ffi.EINVAL
    assert got.value == 77 and w.value == 5 and not out.any() and not ep.view(np.uint64).any()
    after = g.detect_read(), g.detect_log(), g.detect_open()
    assert g.detect_count() == (3, 0)
    for a, b, per in zip(after, before, (64, 8, 8)):
        same_words(a, b, per, "after the refused calls", str)
    g.close()
    t = serf_amd.create(256, fanout=3)                                   # inside a tick
    t.detect_start(0, 1, 8, 4)
    t.step(2)
    t.step_begin()
    for call in (lambda: t.detect_start(0, 1, 8, 4), t.detect_count, lambda: t.detect_read(0, 1), t.detect_log_count,
                 lambda: t.detect_log(0, 0), t.detect_open, t.detect_stop):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                                   # a handle destroyed with a log running
    g.detect_start(0, 1, 4, 300)
    g.step(6)
    assert g.detect_count() == (4, 2) and g.detect_read()["tick"].tolist() == [1, 2, 3, 4]
    g.close()
