"""The rumour catalogue of the HIP library (include/serf_sim_catalog.h) against the reference model (tests/catalog_model.py) on
the oracle stepped one tick at a time: the scenarios of tests/test_catalog.py.  The HIP handle advances in long sim_step calls
and is read once at the end; every operation is injected up front.  Every sample word, the whole registry, catalog_live and
catalog_now are compared exactly, and the digest equals the oracle's in every test."""
import numpy as np
import pytest

import serf_amd
from serf_amd import _ffi
from tests import test_catalog as tc
from tests import test_ledger as tl
from tests import test_observer_shapes as shapes
from tests.catalog_model import CatalogModel
from tests.ledger_model import LedgerModel
from tests.series_model import SeriesModel
from tests.test_ledger_gpu import assert_same as ledger_same
from tests.test_series_gpu import assert_same as series_same

pytestmark = pytest.mark.gpu
SW = _ffi.CATALOG_SAMPLE_WORDS


def words(a):
    return np.ascontiguousarray(np.atleast_1d(np.asarray(a))).view(np.uint64).reshape(-1)


def same_words(got, want, what, per, names=None):
    """Two arrays of records of `per` words, word for word; the first difference is named."""
    g, w = words(got).reshape(-1, per), words(want).reshape(-1, per)
    assert g.shape == w.shape, f"{what}: {g.shape[0]} records, the model has {w.shape[0]}"
    bad = np.argwhere(g != w)
    assert not len(bad), f"{what}: word {bad[0][1]} of record {bad[0][0]}: HIP {g[tuple(bad[0])]} != model {w[tuple(bad[0])]}"


def same_catalogue(g, r, what, kinds_mask=tc.ALL):
    """Everything a running catalogue on handle g says against the model's run r (tests/test_catalog.run)."""
    assert g.catalog_count() == r["count"], what
    same_words(g.catalog_read(), r["samples"], what + ": samples", SW)
    same_words(g.catalog_list(), r["registry"], what + ": registry", 8)
    same_words(g.catalog_live(), r["live"], what + ": live table", 8)
    hdr, live = g.catalog_now(kinds_mask)
    same_words(hdr, r["now"][0], what + ": catalog_now's sample", SW)
    same_words(live, r["now"][1], what + ": catalog_now's table", 8)
    same_words(g.catalog_read(), r["samples"], what + ": samples behind catalog_now", SW)       # it did not touch the running one
    assert g.digest() == r["oracle"].digest(), what


def hip_run(name, arg=None):
    n, kw, drive, start = tc.scenario(name, arg)
    g = serf_amd.create(n, **kw)
    g.catalog_start(**start)
    drive(g, g.step)
    return g


def same_run(name, arg=None):
    r = tc.run(name, arg)
    g = hip_run(name, arg)
    same_catalogue(g, r, f"{name} {arg}", tc.scenario(name, arg)[3]["kinds_mask"])
    return g, r


# ---- 1. cluster sizes ----
@pytest.mark.parametrize("fan", sorted(shapes.FANOUTS))
@pytest.mark.parametrize("n", tc.SHAPE_SIZES)
def test_cluster_sizes(hiplib, n, fan):
    """One wave; a ragged wave and two workgroups; 17 tables, one merge level; 33 tables, two levels with a last group of one."""
    g, r = same_run("ragged", (n, fan))
    assert r["samples"]["live"].max() >= 3 and r["samples"]["queued"].max() > n // 2
    g.close()


def test_second_pass(hiplib):
    """SER_CAP + 65 nodes: the scan's pass loop takes a second turn, of one whole wave and one lane; 1 024 tables, 32, 1."""
    assert tc.tables(shapes.SERIES_N) == [1024, 32, 1]
    g, r = same_run("second_pass")
    s = r["samples"]
    assert s["tick"].tolist() == [1, 5, 9] and s["live"][0] >= 1 and s["running"][-1] == shapes.SERIES_N - 1
    g.close()


@pytest.mark.parametrize("fan", sorted(shapes.FANOUTS))
def test_an_idle_cluster(hiplib, fan):
    g, r = same_run("idle", (65, fan))
    s = r["samples"]
    assert s["running"][-1] == 0 and s["live"][-1] == 0 and len(r["live"]) == 0 and not s["queued"][shapes.IDLE_CRASH:].any()
    g.close()


# ---- 2. the ledger's scenarios ----
@pytest.mark.parametrize("name,arg", [("dies", None), ("lives", None), ("twice", None), ("census", "krandomnodes"), ("census", "bijection")])
def test_ledger_scenarios(hiplib, name, arg):
    g, r = same_run(name, arg)
    assert len(r["registry"]) >= 4
    g.close()


# ---- 3. deep queues, two pages, all seven kinds; the GPU's own ledger on what the catalogue found ----
def test_deep_queues_and_the_ledger_on_what_was_found(hiplib):
    g, r = same_run("deep")
    g.close()
    s = r["samples"]
    assert (s["live_by_kind"].max(axis=0) > 0).all()
    # the tick with the most live identities, on a second handle: sim_ledger_now on 64 of those sim_catalog_live returns
    most = int(np.argmax(s["live"]))
    g = serf_amd.create(tl.DEEP_N, **tl.DEEP_KW)
    g.catalog_start()
    tl.deep_drive(g, lambda k: g.step(most + 1))
    live = g.catalog_live()
    assert len(live) == s["live"][most] > 64
    pick = live[:: len(live) // 64][:64]
    hdr, rec = g.ledger_now([tc.entry_of((int(x["id"]), int(x["val"]))) for x in pick])
    for f in ("id", "val", "holders", "queued", "transmits", "in_flight", "fresh"):
        assert rec[f].tolist() == pick[f].tolist(), f
    assert [int(hdr[f]) for f in ("queued", "in_flight", "packets", "transmits")] == [int(s[f][most]) for f in ("queued", "in_flight", "packets", "transmits")]
    g.close()


def test_two_accusers_in_one_queue_and_a_restore_under_a_running_catalogue(hiplib):
    """The made state of tests/test_catalog.two_accusers: one identity, holders 1, queued 2.  The catalogue is started on the
    fresh handle, sim_restore leaves it running: its samples go on behind the restored tick."""
    image, tick, node, subject = tc.two_accusers()
    o, (w, table), samples, reg, live = tc.two_accusers_run()
    g = serf_amd.create(tl.DEEP_N, **tl.DEEP_KW)
    g.catalog_start()
    g.restore(image)
    hdr, now = g.catalog_now()
    same_words(hdr, w, "right behind the restore: sample", SW)
    same_words(now, table, "right behind the restore: table", 8)
    at = now["id"].tolist().index(subject | (_ffi.K_SUSPECT << 32))
    assert (int(now["holders"][at]), int(now["queued"][at])) == (1, 2)
    assert g.catalog_count() == (0, 0)
    g.step(tc.TWO_TICKS)
    assert g.catalog_count() == (tc.TWO_TICKS, 0)
    same_words(g.catalog_read(), samples, "behind a restore: samples", SW)
    same_words(g.catalog_list(), reg, "behind a restore: registry", 8)
    same_words(g.catalog_live(), live, "behind a restore: live table", 8)
    assert g.digest() == o.digest()
    g.close()


def test_member_kinds_only(hiplib):
    g, r = same_run("members")
    assert {int(x) >> 32 for x in g.catalog_list()["id"]} == {5, 6, 7}
    g.close()


# ---- 4. the overflow boundary, the full registry, crash and revive ----
def test_256_identities_fit(hiplib):
    g, r = same_run("over", (256, 0))
    s = g.catalog_read()
    assert s["live"][2] == 256 and not s["overflow"].any()
    g.close()


def test_257_identities_are_flagged_and_the_next_sample_is_exact_again(hiplib):
    r = tc.run("over", (200, 57))
    n, kw, drive, start = tc.scenario("over", (200, 57))
    g = serf_amd.create(n, **kw)
    g.catalog_start(**start)
    for i, node in enumerate(tc.over_origins(257)):
        g.inject(2 if i < 200 else 4, _ffi.OP_USER_EVENT, node, 0x54000000 + i, 64)
    g.step(4)
    before = (g.catalog_list(), g.catalog_live())
    assert len(before[0]) == len(before[1]) == 200
    g.step(1)                                                     # behind tick 4: 257
    s = g.catalog_read()
    assert s["overflow"].tolist() == [0, 0, 0, 0, 1] and s["live"][-1] == 0 and s["queued"][-1] > 0
    same_words(g.catalog_list(), before[0], "the registry behind an overflowed sample", 8)
    assert len(g.catalog_live()) == 0
    hdr, now = g.catalog_now()
    assert hdr["overflow"] == 1 and len(now) == 0
    g.step(tc.OVER_TICKS - 5)
    same_catalogue(g, r, "257")
    s = g.catalog_read()
    assert s["overflow"][5] == 0 and s["died"][5] + s["live"][5] == 200 + s["new"][5] and s["died"][5] > 0
    g.close()


def test_a_full_registry(hiplib):
    g, r = same_run("registry")
    assert len(g.catalog_list()) == tc.REG_MAX and g.catalog_read()["ids_lost"][-1] == 4
    same_words(g.catalog_list(2, 3), r["registry"][2:5], "a partial list", 8)
    assert len(g.catalog_list(tc.REG_MAX)) == 0
    g.close()


def test_crash_and_revive(hiplib):
    g, r = same_run("crash")
    assert g.catalog_list()["revivals"].tolist() == [1]
    g.close()


# ---- 5. rules, other observers ----
def test_period_first_tick_capacity_and_restart(hiplib):
    n, kw, drive, _ = tc.scenario("deep")
    first, period, ticks = 5, 7, 60
    due = len(range(first, ticks, period))
    o = tl.maker(n, kw)()
    g = serf_amd.create(n, **kw)
    m = CatalogModel(o)
    for s in (o, g):
        tl.sc.apply_schedule(s, tl.sc.schedule(n, 40, rate=2.0, seed=524, max_member_subjects=40))
    m.start(tc.ALL, 40, first, period, due - 3)
    g.catalog_start(tc.ALL, 40, first, period, due - 3)
    m.step(ticks)
    g.step(ticks)
    assert g.catalog_count() == m.count() == (due - 3, 3)
    with pytest.raises(_ffi.SimError) as ei:
        g.catalog_start()                                          # one catalogue at a time
    assert ei.value.code == _ffi.ESTATE
    same_words(g.catalog_read(), m.read(), "period 7", SW)
    same_words(g.catalog_read(2, 3), m.read(2, 3), "a partial read", SW)
    same_words(g.catalog_list(), m.list(), "period 7: registry", 8)
    assert len(m.list()) == 40 and m.read()["ids_lost"][-1] > 0
    g.catalog_stop()
    m.stop()
    assert g.catalog_count() == (0, 0)
    m.start(tc.MEMBERS, 4096, 0, 2, 5)                             # a first tick that has passed: now; an empty registry again
    g.catalog_start(tc.MEMBERS, 4096, 0, 2, 5)
    m.step(7)
    g.step(7)
    assert g.catalog_count() == m.count() == (4, 0)
    same_words(g.catalog_read(), m.read(), "restarted", SW)
    same_words(g.catalog_list(), m.list(), "restarted: registry", 8)
    assert g.digest() == o.digest()
    g.close()


def test_next_to_the_other_observers(hiplib):
    """deep with a series, the ledger of tests/test_ledger.py's entries and the catalogue on one handle: each equals its own
    model, which does not know the others."""
    o_l, entries, want_ledger = tl.deep_oracle()[:3]
    r = tc.run("deep")
    o = tl.maker(tl.DEEP_N, tl.DEEP_KW)()
    sm = SeriesModel(o)
    sm.start(0, 3, 1000)
    tl.deep_drive(o, sm.step)
    g = serf_amd.create(tl.DEEP_N, **tl.DEEP_KW)
    g.series_start(0, 3, 1000)
    g.ledger_start(entries, 0, 1, tl.DEEP_TICKS)
    g.census_start(0, 1, tl.DEEP_TICKS, 8)
    g.catalog_start(**tc.scenario("deep")[3])
    tl.deep_drive(g, g.step)
    same_catalogue(g, r, "next to the others")
    ledger_same(g.ledger_read(), want_ledger, "a ledger next to the catalogue")
    series_same(g.series_read(), sm.read(), "a series next to the catalogue")
    assert g.census_count() == (tl.DEEP_TICKS, 0)
    g.close()


# ---- 6. errors ----
def test_errors_leave_everything_as_it_was(hiplib):
    n, kw = 4096, tl.census_kw("krandomnodes")
    sh = serf_amd.create(n, force_sharded=True, **kw)            # a shard has no catalogue
    for call in (sh.catalog_start, sh.catalog_count, lambda: sh.catalog_read(0, 0), sh.catalog_stop, sh.catalog_list, sh.catalog_live,
                 sh.catalog_now):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    sh.close()
    g = serf_amd.create(tc.REG_N, **tc.REG_KW)
    assert g.catalog_count() == (0, 0)
    for call in (lambda: g.catalog_read(0, 0), g.catalog_stop, g.catalog_list, g.catalog_live):      # no catalogue yet
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    for args in ((0, 8), (1, 8), (0x100, 8), (0x1FE, 8), (0xFF, 8), (tc.ALL, 0), (tc.ALL, _ffi.CATALOG_MAX + 1)):
        with pytest.raises(_ffi.SimError) as ei:
            g.catalog_start(*args)
        assert ei.value.code == _ffi.EINVAL and g.catalog_count() == (0, 0), args
    for mask in (0, 1, 0x100):
        with pytest.raises(_ffi.SimError) as ei:
            g.catalog_now(mask)
        assert ei.value.code == _ffi.EINVAL
    for args in ((0, 0, 8), (0, 1, 0), (0, 1, _ffi.CATALOG_MAX_SAMPLES + 1)):
        with pytest.raises(_ffi.SimError) as ei:
            g.catalog_start(tc.ALL, 8, *args)
        assert ei.value.code == _ffi.EINVAL and g.catalog_count() == (0, 0)
    f, C = g.lib.f, _ffi.C
    got, total = C.c_uint32(77), C.c_uint32(78)
    buf, hdr = np.zeros(8 * 256, np.uint64), np.zeros(SW, np.uint64)
    assert f["catalog_start"](None, tc.ALL, 8, 0, 1, 8) == _ffi.EINVAL
    assert f["catalog_now"](g.h, tc.ALL, None, buf.ctypes.data, buf.size, C.byref(got)) == _ffi.EINVAL
    assert f["catalog_now"](g.h, tc.ALL, hdr.ctypes.data, None, buf.size, C.byref(got)) == _ffi.EINVAL
    assert f["catalog_now"](g.h, tc.ALL, hdr.ctypes.data, buf.ctypes.data, buf.size, None) == _ffi.EINVAL
    for x in range(4):
        g.inject(1, _ffi.OP_USER_EVENT, 10 + x, 0x700 + x, 64)
    g.catalog_start(tc.ALL, 8, 0, 1, 8)
    g.step(3)
    assert g.catalog_count() == (3, 0)
    before = (g.catalog_read(), g.catalog_list(), g.catalog_live())
    assert before[0]["tick"].tolist() == [1, 2, 3] and len(before[1]) == len(before[2]) == 4
    for first, cnt in ((0, 4), (3, 1), (4, 0)):                   # beyond `taken`
        with pytest.raises(_ffi.SimError) as ei:
            g.catalog_read(first, cnt)
        assert ei.value.code == _ffi.EINVAL
    with pytest.raises(_ffi.SimError) as ei:
        g.catalog_list(5, 1)                                       # beyond the registry
    assert ei.value.code == _ffi.EINVAL
    small = np.zeros(2 * SW, np.uint64)
    assert f["catalog_read"](g.h, 0, 3, small.ctypes.data, small.size, C.byref(got)) == _ffi.EINVAL      # a buffer one sample short
    assert f["catalog_read"](g.h, 0, 2, None, small.size, C.byref(got)) == _ffi.EINVAL
    assert f["catalog_list"](g.h, 0, 4, buf.ctypes.data, 8 * 3, C.byref(got), C.byref(total)) == _ffi.EINVAL
    assert f["catalog_list"](g.h, 0, 4, None, buf.size, C.byref(got), C.byref(total)) == _ffi.EINVAL
    assert f["catalog_list"](g.h, 0, 4, buf.ctypes.data, buf.size, C.byref(got), None) == _ffi.EINVAL
    assert f["catalog_live"](g.h, buf.ctypes.data, 8 * 3, C.byref(got)) == _ffi.EINVAL
    assert f["catalog_live"](g.h, None, buf.size, C.byref(got)) == _ffi.EINVAL and f["catalog_live"](g.h, buf.ctypes.data, buf.size, None) == _ffi.EINVAL
    assert f["catalog_now"](g.h, tc.ALL, hdr.ctypes.data, buf.ctypes.data, 8 * 3, C.byref(got)) == _ffi.EINVAL
    assert f["catalog_count"](g.h, None, C.byref(total)) == _ffi.EINVAL and f["catalog_count"](None, C.byref(got), C.byref(total)) == _ffi.EINVAL
    assert (got.value, total.value) == (77, 78) and not buf.any() and not small.any() and not hdr.any()
    assert f["catalog_list"](g.h, 1, 100, buf.ctypes.data, buf.size, C.byref(got), C.byref(total)) == 0 and (got.value, total.value) == (3, 4)
    after = (g.catalog_read(), g.catalog_list(), g.catalog_live())
    for a, b, per in zip(after, before, (SW, 8, 8)):
        same_words(a, b, "behind the refused calls", per)
    g.close()
    t = serf_amd.create(256, fanout=3)                            # inside a tick
    t.catalog_start()
    t.step(2)
    t.step_begin()
    for call in (t.catalog_start, t.catalog_count, lambda: t.catalog_read(0, 1), t.catalog_stop, t.catalog_list, t.catalog_live, t.catalog_now):
        with pytest.raises(_ffi.SimError) as ei:
            call()
        assert ei.value.code == _ffi.ESTATE
    t.close()
    g = serf_amd.create(256, fanout=3)                            # a handle destroyed with a catalogue running
    g.catalog_start(tc.ALL, 8, 0, 1, 4)
    g.step(6)
    assert g.catalog_count() == (4, 2) and g.catalog_read()["tick"].tolist() == [1, 2, 3, 4]
    g.close()
