"""The query board of the HIP library (include/serf_sim_qboard.h) against the reference model (tests/qboard_model.py) on the oracle
stepped one tick at a time: the scenarios of tests/test_qboard.py at the sizes where qboard_count_kernel can go wrong (an odd number
of bitmap words, ragged last waves, three nodes, the second turn of the pass loop), the table's edges, filters and tags, liveness,
the sampling rules, loss, neutrality, the errors, the rankings.  The HIP handle advances in long sim_step calls and is read once at
the end; every operation is scheduled up front; every word of the samples, of the three reads and of qboard_now is compared
exactly, and the digest equals the oracle's in every test."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_qboard as tq
from tests.qboard_model import CLOSED, EW, HW, OPEN, WAITING, QBoardModel, Script, q_timeout

pytestmark = pytest.mark.gpu
ACK, RESP = tq.ACK, tq.RESP


def words(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1)


def same_samples(got, want, what):
    """(headers, records) of the library against the model's, word for word."""
    (gh, gr), (wh, wr) = got, want
    assert gh.shape == wh.shape and gr.shape == wr.shape, f"{what}: {gh.shape} {gr.shape} != {wh.shape} {wr.shape}"
    for f in _ffi.QBOARD_HEADER_DTYPE.names:
        bad = np.nonzero(gh[f] != wh[f])[0]
        assert not len(bad), f"{what}: header.{f} of sample {bad[0]}: HIP {gh[f][bad[0]]} != model {wh[f][bad[0]]}"
    for f in _ffi.QBOARD_ENTRY_DTYPE.names:
        bad = np.argwhere(gr[f] != wr[f])
        assert not len(bad), f"{what}: {f} of sample {bad[0][0]}, entry {bad[0][1]}: HIP {gr[f][tuple(bad[0])]} != model {wr[f][tuple(bad[0])]}"
    assert words(gh).tolist() == words(wh).tolist() and words(gr).tolist() == words(wr).tolist()


def same_records(got, want, what):
    for f in want.dtype.names:
        bad = np.argwhere(np.asarray(got[f] != want[f]))
        assert not len(bad), f"{what}: {f} at {bad[0].tolist()}: HIP {got[f][tuple(bad[0])]} != model {want[f][tuple(bad[0])]}"
    assert words(got).tolist() == words(want).tolist(), what


def same_reads(g, m, what, top_ks=(1, 7, 64), nodes=True):
    """The silent lists of every entry for both bitmaps, whole and with a cap below the total; every node's record; the ranking
    for both orders; qboard_now of the board's ids and of one nobody scheduled."""
    n = int(g.cfg.n_nodes)
    for e in range(len(m.ids)):
        for which in (0, 1):
            ids, total = g.qboard_silent(e, which)
            wids, wtotal = m.silent(e, which)
            assert total == wtotal and ids.tolist() == wids.tolist(), f"{what}: silent({e}, {which})"
            cap = max(0, wtotal - 3) if wtotal > 3 else wtotal // 2
            ids, total = g.qboard_silent(e, which, cap)
            assert total == wtotal and ids.tolist() == wids[:cap].tolist(), f"{what}: silent({e}, {which}), cap {cap}"
    every = m.nodes()
    if nodes:
        same_records(g.qboard_nodes(), every, f"{what}: every node's record")
        if n > 5:
            same_records(g.qboard_nodes(2, 3), every[2:5], f"{what}: nodes 2 .. 4")
            assert len(g.qboard_nodes(n, 0)) == 0
    for rank_by in (_ffi.QBOARD_BY_SILENT_ACK, _ffi.QBOARD_BY_SILENT_RESP):
        for k in top_ks:
            wtop = m.top(k, rank_by)
            if nodes:
                top, got_every = g.qboard_top(k, rank_by, nodes=True)
                same_records(got_every, every, f"{what}: every node's record behind the ranking")
                same_records(top, wtop, f"{what}: top {k} by {rank_by}")
            same_records(g.qboard_top(k, rank_by), wtop, f"{what}: top {k} by {rank_by} without nodes")
    ask = list(m.ids)[::-1][:_ffi.QBOARD_MAX - 1] + [0x7FFFFFF1]
    (gh, gr), (wh, wr) = g.qboard_now(ask), m.now(ask)
    assert words(gh).tolist() == words(wh).tolist() and words(gr).tolist() == words(wr).tolist(), f"{what}: qboard_now"
    assert not gr["new_acks"].any() and not gr["t_first"].any() and gr["state"][-1] == WAITING


def same_run(n, kw, scenario, run, what, before=0, ticks=None, **start):
    """The scenario on the HIP library, read once at the end, against the cached oracle run."""
    o, m, want = run["o"], run["m"], run["samples"]
    g = serf_amd.create(n, **kw)
    scenario(Script(g))
    if before:
        g.step(before)
    g.qboard_start(run["ids"], **start)
    g.step(int(o.tick) - before if ticks is None else ticks)
    assert g.tick == o.tick and g.qboard_count() == (len(want[0]), m.count()[1])
    same_samples(g.qboard_read(), want, what)
    same_reads(g, m, what, nodes=n <= 4096)
    assert g.digest() == o.digest(), what
    return g


# ---- 1. sizes: an odd number of bitmap words, ragged waves, more than one workgroup; the table's edges, filters, tags, crashes ----
@pytest.mark.parametrize("n", (65, 96))
def test_odd_word_count(hiplib, n):
    """Three words a bitmap: the last wave's second word is the response bitmap's first.  Node 0 responds to query 256 (its
    response bit is bit 0 of that word) and to nothing else in its residue: read unguarded and unmasked it would be an ack of node
    n' = 96 .. 127.  Query 255's response bitmap is the last of qbits: its word 3 is past the allocation."""
    run = tq.full_run(n)
    tq.check_full(n, run)
    assert (n + 31) // 32 == 3
    hdr, rec = run["samples"]
    assert rec["responses"][8, 0] > n // 2 and rec["acks"][:, 0].max() <= n, "more than half the nodes responded: some of nodes 0 .. 31 did"
    same_run(n, tq.full_kw(n), lambda sc: tq.full(sc, n), run, f"full({n})").close()


@pytest.mark.parametrize("n", (33, 64, 97, 257))
def test_other_small_sizes(hiplib, n):
    run = tq.full_run(n)
    tq.check_full(n, run)
    same_run(n, tq.full_kw(n), lambda sc: tq.full(sc, n), run, f"full({n})").close()


@pytest.mark.parametrize("n", (65, 257))
def test_the_bijection_and_four_vshards(hiplib, n):
    run = tq.full_run(n, tq.BIJECTION)
    tq.check_full(n, run)
    same_run(n, tq.full_kw(n, tq.BIJECTION), lambda sc: tq.full(sc, n), run, f"full({n}) bijection").close()


def test_four_vshards_on_one_handle(hiplib):
    n = 256
    kw = dict(tq.full_kw(n), vshards=4)
    run = tq.model_run(n, kw, lambda sc: tq.full(sc, n), tq.FULL_IDS, tq.full_ticks(n))
    tq.check_full(n, run)
    same_run(n, kw, lambda sc: tq.full(sc, n), run, "full(256) vshards 4").close()


@pytest.mark.parametrize("name", ("tiny", "crowd", "idle", "late"))
def test_three_nodes_64_entries_and_nobody_running(hiplib, name):
    n, kw, scenario, ids, ticks = tq.SMALL[name]
    same_run(n, kw, scenario, tq.small_run(name), name).close()


def test_a_threshold_first_met_behind_the_deadline_latches_nothing(hiplib):
    """The `late` scenario with a board started behind node 11's revive: answered == eligible is first met in a closed sample."""
    n, kw, scenario, ids, ticks = tq.LATE
    run = tq.model_run(n, kw, scenario, ids, ticks - 24, before=24)
    col = run["samples"][1][:, 0]
    assert col["t_half"][0] == 25 and not col["t_all"].any() and (col["answered"][-4:] == col["eligible"][-4:]).all()
    same_run(n, kw, scenario, run, "late, started at tick 24", before=24).close()


# ---- 2. sampling ----
def test_period_3_a_late_first_tick_and_a_full_buffer(hiplib):
    n, first, period = 65, 7, 3
    due = len(range(first, tq.full_ticks(n), period))
    run = tq.model_run(n, tq.full_kw(n), lambda sc: tq.full(sc, n), tq.FULL_IDS, tq.full_ticks(n), first=first, period=period,
                       capacity=due - 3)                   # (a run of this test's own: its oracle goes on below)
    assert run["m"].count() == (due - 3, 3)
    g = same_run(n, tq.full_kw(n), lambda sc: tq.full(sc, n), run, "period 3", first_tick=first, period=period, capacity=due - 3)
    same_samples(g.qboard_read(2, 3), run["m"].read(2, 3), "a partial read")
    assert g.qboard_read(1, 0)[0].shape == (0,)
    with pytest.raises(_ffi.SimError) as ei:
        g.qboard_start([1], 0, 1, 8)                       # one board at a time
    assert ei.value.code == _ffi.ESTATE and g.qboard_count() == (due - 3, 3)
    g.qboard_stop()
    with pytest.raises(_ffi.SimError) as ei:
        g.qboard_read(0, 0)
    assert ei.value.code == _ffi.ESTATE and g.qboard_count() == (0, 0)
    g.qboard_start([256, 261], 0, 2, 5)                    # a first tick that has passed: now; a new board starts from nothing
    m = QBoardModel(run["o"], run["script"])
    m.start([256, 261], 0, 2, 5)
    m.step(7)
    g.step(7)
    assert g.qboard_count() == m.count() == (4, 0)
    same_samples(g.qboard_read(), m.read(), "restarted")
    assert m.read()[1]["new_acks"][0].tolist() == m.read()[1]["acks"][0].tolist()
    assert g.digest() == run["o"].digest()
    g.close()


def test_one_step_call_against_single_steps_and_reads_in_between(hiplib):
    n = 97
    run = tq.full_run(n)
    ticks = tq.full_ticks(n)
    a, b = serf_amd.create(n, **tq.full_kw(n)), serf_amd.create(n, **tq.full_kw(n))
    for g in (a, b):
        tq.full(Script(g), n)
        g.qboard_start(tq.FULL_IDS, 0, 1, ticks)
    a.step(ticks)
    for t in range(ticks):
        b.step(1)
        if t % 7 == 3:
            b.qboard_silent(t % len(tq.FULL_IDS), t & 1, 5)
            b.qboard_nodes(1, 9)
            b.qboard_top(3, _ffi.QBOARD_BY_SILENT_RESP, nodes=True)
            b.qboard_now([5, 256])
            b.qboard_read(0, 1)
    same_samples(a.qboard_read(), b.qboard_read(), "step(n) against n step(1) with reads between them")
    same_samples(b.qboard_read(), run["samples"], "the model's samples")
    assert a.digest() == b.digest() == run["o"].digest()
    a.close()
    b.close()


def test_a_board_started_while_queries_run(hiplib):
    n = 65
    run = tq.full_run(n, before=9)
    assert run["samples"][1]["new_acks"][0, 0] == run["samples"][1]["acks"][0, 0] > 0
    same_run(n, tq.full_kw(n), lambda sc: tq.full(sc, n), run, "started at tick 9", before=9).close()


def test_boards_and_a_restore(hiplib):
    """A board started on a restored handle, and a board that runs when its handle is restored (the restore leaves it as it is);
    the image holds no board."""
    n, at = 65, 9
    kw = tq.full_kw(n)
    src = tq.make(n, kw)
    sc0 = Script(src)
    tq.full(sc0, n)
    src.step(at)
    img = src.snapshot()
    for started_before in (False, True):
        o, g = tq.make(n, kw), serf_amd.create(n, **kw)
        sc = Script()
        sc.ops, sc.tags0 = list(sc0.ops), sc0.tags0          # what the image's tables and schedule come from
        m = QBoardModel(o, sc)
        if started_before:
            m.start(tq.FULL_IDS)
            g.qboard_start(tq.FULL_IDS)
        o.restore(img)
        g.restore(img)
        if not started_before:
            m.start(tq.FULL_IDS)
            g.qboard_start(tq.FULL_IDS)
        assert g.tick == o.tick == at and g.qboard_count() == (0, 0)
        m.step(30)
        g.step(30)
        assert g.snapshot().tobytes() == o.snapshot().tobytes()
        want = m.read()
        assert want[0]["tick"][0] == at + 1 and want[1]["state"][0].tolist() == [OPEN, OPEN, OPEN, WAITING, WAITING]
        same_samples(g.qboard_read(), want, f"restore, started before: {started_before}")
        same_reads(g, m, "restore", top_ks=(7,))
        assert g.digest() == o.digest()
        g.close()
        o.close()
    src.close()


# ---- 3. loss ----
@pytest.mark.parametrize("relay_factor,fan", tq.LOSS_VARIANTS)
def test_loss_with_and_without_relays(hiplib, relay_factor, fan):
    """4 096 nodes, a third of the packets lost: exactness is the assertion; the shares are printed for profiles/r16_qboard.md."""
    run = tq.loss_run(relay_factor, fan)
    hdr, rec = run["samples"]
    last = rec[q_timeout(tq.LOSS_N)]
    print(f"loss 0.3 relay {relay_factor} {fan}: answered / eligible at the last open sample {last['answered'].tolist()} / {last['eligible'].tolist()}, "
          f"t_half {last['t_half'].tolist()} t_90 {last['t_90'].tolist()} t_all {last['t_all'].tolist()}")
    assert last["state"].tolist() == [OPEN, OPEN] and last["eligible"][1] == tq.LOSS_N // 2
    g = serf_amd.create(tq.LOSS_N, **tq.loss_kw(fan))
    g.init_tags([x % 2 for x in range(tq.LOSS_N)])
    tq.lossy(Script(g), relay_factor)
    g.qboard_start([700, 701])
    g.step(int(run["o"].tick))
    same_samples(g.qboard_read(), run["samples"], f"loss, relay {relay_factor}, {fan}")
    same_reads(g, run["m"], "loss", top_ks=(64,))
    assert g.digest() == run["o"].digest()
    g.close()


# ---- 4. the second turn of the pass loop ----
def test_second_pass(hiplib):
    """QBOARD_GRID * BLOCK + 65 nodes: the pass loop of qboard_count_kernel takes a second turn, of one whole wave and one lane;
    the query's origin, a crashed node and silent nodes lie in that pass."""
    tq.test_the_cap_is_the_sources()
    n = tq.SECOND_N
    assert n == 262209
    run = tq.second_pass_run()
    hdr, rec = run["samples"]
    assert hdr["tick"].tolist() == [1, 5, 9] and hdr["running"].tolist() == [n, n - 1, n - 1]
    assert rec["origin"][-1, 0] == n - 3 and rec["state"][-1, 0] == OPEN and 100 < rec["answered"][-1, 0] < n - 1000
    ids, total = run["m"].silent(0, 0)
    assert total == rec["silent"][-1, 0] and (ids >= tq.QBOARD_GRID * tq.BLOCK).sum() >= 1, "no silent node in the second pass"
    same_run(n, tq.SECOND_KW, tq.second, run, "second pass", period=tq.SECOND_PERIOD, capacity=100).close()


# ---- 5. neutrality ----
def test_a_running_board_changes_no_protocol_state(hiplib):
    n = 257
    kw = tq.full_kw(n)
    with_board, without = serf_amd.create(n, **kw), serf_amd.create(n, **kw)
    for g in (with_board, without):
        for x in (0, 5, n - 1):
            g.watch(x)
        tq.full(Script(g), n)
    with_board.qboard_start(tq.FULL_IDS, 0, 1, 1 << 10)
    ticks = tq.full_ticks(n)
    for g in (with_board, without):
        g.step(ticks)
    assert with_board.qboard_count() == (ticks, 0) and without.qboard_count() == (0, 0)
    assert with_board.digest() == without.digest()       # (three nodes are watched: a watched node's row says so, the plain oracle run's digest is another)
    ev = with_board.drain_events()
    assert ev == without.drain_events() and len(ev) >= 5
    assert with_board.cluster_stats() == without.cluster_stats()
    assert with_board.snapshot().tobytes() == without.snapshot().tobytes(), "an image holds no board"
    for which in (_ffi.ARR_ROWS, _ffi.ARR_QUEUE, _ffi.ARR_QRING):
        assert with_board.dump(which).tobytes() == without.dump(which).tobytes(), f"dump {which}"
    for call in (lambda: without.qboard_read(0, 0), without.qboard_stop, lambda: without.qboard_silent(0), without.qboard_nodes, without.qboard_top):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    hdr, rec = without.qboard_now(tq.FULL_IDS)                # qboard_now needs no board
    ref = tq.full_run(n)["samples"][1][-1]
    assert rec["acks"].tolist() == ref["acks"].tolist() and rec["state"].tolist() == [CLOSED, CLOSED, WAITING, CLOSED, WAITING]
    with_board.close()
    without.close()


# ---- 6. errors and states ----
def test_errors_leave_everything_as_it_was(hiplib):
    n = 257
    kw = tq.full_kw(n)
    ok = [256, 5, 261]
    sh = serf_amd.create(n, force_sharded=True, **kw)      # a shard has no board
    every = lambda s: (lambda: s.qboard_start(ok), s.qboard_count, lambda: s.qboard_read(0, 0), s.qboard_stop, lambda: s.qboard_now(ok),
                       lambda: s.qboard_silent(0), lambda: s.qboard_nodes(0, 1), s.qboard_top)
    for call in every(sh):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    g = serf_amd.create(n, **kw)
    assert g.qboard_count() == (0, 0)
    for call in (every(g)[2], every(g)[3]) + every(g)[5:]:                # no board yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    bad = [[], list(range(1, 66)), [0], [5, 0], [5, 6, 5], ok + [256]]
    for ids in bad:
        for call in (lambda: g.qboard_start(ids, 0, 1, 8), lambda: g.qboard_now(ids)):
            with pytest.raises(_ffi.SimError) as ei:
                call()
            assert ei.value.code == _ffi.EINVAL and g.qboard_count() == (0, 0), ids
    for args in ((0, 0, 8), (0, 1, 0), (0, 1, _ffi.QBOARD_MAX_SAMPLES + 1)):
        with pytest.raises(_ffi.SimError) as ei:
            g.qboard_start(ok, *args)
        assert ei.value.code == _ffi.EINVAL and g.qboard_count() == (0, 0)
    f = g.lib.f
    u = _ffi.C.c_uint32
    arr = (u * 3)(*ok)
    buf = np.zeros(4096, np.uint64)
    assert f["qboard_start"](g.h, None, 3, 0, 1, 8) == _ffi.EINVAL and f["qboard_start"](None, arr, 3, 0, 1, 8) == _ffi.EINVAL
    assert f["qboard_now"](g.h, None, 3, buf.ctypes.data) == _ffi.EINVAL and f["qboard_now"](g.h, arr, 3, None) == _ffi.EINVAL
    assert f["qboard_now"](None, arr, 3, buf.ctypes.data) == _ffi.EINVAL
    # arguments that can be judged without a board are SIM_EINVAL before "no board" is SIM_ESTATE
    a, b = u(77), u(78)
    ref = _ffi.C.byref
    assert f["qboard_silent"](g.h, 0, 0, None, 4, ref(a), ref(b)) == _ffi.EINVAL
    assert f["qboard_silent"](g.h, 0, 0, buf.ctypes.data, 4, None, ref(b)) == _ffi.EINVAL
    assert f["qboard_silent"](g.h, 0, 0, buf.ctypes.data, 4, ref(a), None) == _ffi.EINVAL
    assert f["qboard_silent"](g.h, 0, 2, buf.ctypes.data, 4, ref(a), ref(b)) == _ffi.EINVAL
    assert f["qboard_nodes"](g.h, 0, 1, None) == _ffi.EINVAL
    for top_k, rank_by in ((0, 0), (65, 0), (8, 2)):
        assert f["qboard_top"](g.h, top_k, rank_by, buf.ctypes.data, None) == _ffi.EINVAL
    assert f["qboard_top"](g.h, 8, 0, None, None) == _ffi.EINVAL
    assert (a.value, b.value) == (77, 78) and not buf.any()
    tq.full(Script(g), n)
    g.qboard_start(ok, 0, 1, 8)
    g.step(5)
    assert g.qboard_count() == (5, 0)
    before = g.qboard_read()
    assert before[0]["tick"].tolist() == [1, 2, 3, 4, 5] and before[1].shape == (5, 3) and before[1]["acks"][-1, 0] > 1
    for ids in bad[:4]:                                                    # bad arguments before "already running"
        with pytest.raises(_ffi.SimError) as ei:
            g.qboard_start(ids, 0, 1, 8)
        assert ei.value.code == _ffi.EINVAL
    with pytest.raises(_ffi.SimError) as ei:
        g.qboard_start(ok, 0, 0, 8)
    assert ei.value.code == _ffi.EINVAL
    with pytest.raises(_ffi.SimError) as ei:
        g.qboard_start(ok, 0, 1, 8)
    assert ei.value.code == _ffi.ESTATE
    for first, cnt in ((0, 6), (5, 1), (6, 0)):                           # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.qboard_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL and g.qboard_count() == (5, 0)
    stride = HW + EW * 3
    got = u(77)
    small = np.zeros(2 * stride, np.uint64)
    assert f["qboard_read"](g.h, 0, 3, small.ctypes.data, small.size, ref(got)) == _ffi.EINVAL          # a buffer one sample short
    assert f["qboard_read"](g.h, 0, 2, None, small.size, ref(got)) == _ffi.EINVAL and f["qboard_read"](g.h, 0, 2, small.ctypes.data, small.size, None) == _ffi.EINVAL
    assert got.value == 77 and not small.any()
    assert f["qboard_count"](g.h, None, ref(b)) == _ffi.EINVAL and f["qboard_count"](g.h, ref(a), None) == _ffi.EINVAL
    assert f["qboard_count"](None, ref(a), ref(b)) == _ffi.EINVAL
    # an entry or nodes out of the running board's range
    out = np.zeros(8 * (n + 1), np.uint64)
    assert f["qboard_silent"](g.h, 3, 0, buf.ctypes.data, 4, ref(a), ref(b)) == _ffi.EINVAL
    for first, cnt in ((n, 1), (0, n + 1), (n - 1, 2), (0xFFFFFFFF, 2)):
        assert f["qboard_nodes"](g.h, first, cnt, out.ctypes.data) == _ffi.EINVAL
    assert f["qboard_top"](g.h, 65, 0, buf.ctypes.data, None) == _ffi.EINVAL and f["qboard_top"](g.h, 8, 2, buf.ctypes.data, None) == _ffi.EINVAL
    assert (a.value, b.value) == (77, 78) and not buf.any() and not out.any()
    ids, total = g.qboard_silent(0, 0, 0)                                  # cap 0: the count alone, no list
    assert len(ids) == 0 and total == before[1]["silent"][-1, 0] > 0
    after = g.qboard_read()
    assert g.qboard_count() == (5, 0) and words(after[0]).tolist() == words(before[0]).tolist() and words(after[1]).tolist() == words(before[1]).tolist()
    g.close()
    t = serf_amd.create(256, fanout=3)                                   # inside a tick
    t.qboard_start(ok, 0, 1, 8)
    t.step(2)
    t.step_begin()
    for call in every(t):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                                   # a handle destroyed with a board running
    g.qboard_start(ok, 0, 1, 4)
    g.step(6)
    assert g.qboard_count() == (4, 2) and g.qboard_read()[0]["tick"].tolist() == [1, 2, 3, 4]
    g.close()


# ---- 7. rankings ----
def tie(sc):
    """Query 40 asks nodes 255 and 256 — the last of one workgroup, the first of the next — and loses its origin in the tick it
    is sent: nobody's ack counts, both stay silent."""
    sc.query(1, 9, 40, ACK | RESP, ids=[255, 256])
    sc.inject(1, _ffi.OP_CRASH, 9)


@pytest.mark.parametrize("n", (257, 3))
def test_rankings_with_every_key_tied(hiplib, n):
    """A board none of whose entries is scheduled: every running node has silent 0; the order is the ids'; at three nodes the
    records beyond the third are zero."""
    kw = dict(tq.KW, view_slots=0 if n == 3 else 16, fanout=2)
    run = tq.model_run(n, kw, lambda sc: sc.inject(1, _ffi.OP_CRASH, 1), [9, 10], 4)
    top = run["m"].top(64, _ffi.QBOARD_BY_SILENT_ACK)
    assert top["id"][:2].tolist() == [0, 2] and top["running"].sum() == min(64, n - 1) and not words(top[n - 1:]).any()
    same_run(n, kw, lambda sc: sc.inject(1, _ffi.OP_CRASH, 1), run, f"all tied ({n})").close()


def test_a_tie_across_the_workgroup_boundary(hiplib):
    n = 257
    run = tq.model_run(n, tq.KW, tie, [40, 41], 12)
    for rank_by in (_ffi.QBOARD_BY_SILENT_ACK, _ffi.QBOARD_BY_SILENT_RESP):
        top = run["m"].top(64, rank_by)
        assert top["id"][:4].tolist() == [255, 256, 0, 1] and top["silent_ack"][:3].tolist() == [1, 1, 0] and top["silent_resp"][:3].tolist() == [1, 1, 0]
    assert run["samples"][1]["acks"].max() == 0 and run["samples"][1]["eligible"][-1].tolist() == [2, 0]
    same_run(n, tq.KW, tie, run, "tie across the boundary").close()
