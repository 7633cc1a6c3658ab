"""The observers — trackers, series, census, roll, ledger, sim_convergence(_many) — across a checkpoint: the part that needs no
GPU.  Every observer header promises "sim_snapshot holds none, sim_restore leaves a running one as it is"; this file owns the
scenarios that put the two together and the conditions that make them non-trivial, and runs them on the CPU oracle with the
reference models.  tests/test_observer_resume_gpu.py drives the HIP library through the same cases and compares word for word.

A case is a scenario of the suite paused at a tick T: before(sim) is what its script does up front, at(o) is asked once, on the
reference oracle at tick T, for the observers' arguments (the trackers' and entries' Lamport times are the oracle's), after(sim,
step) is the rest of the script.  Three oracles per case:

  the image      runs to T and is snapshotted; its image goes into a fresh HIP handle (and into the third oracle)
  the reference  never restores and is never snapshotted: the models are chained on it from tick 0 — the tracker model sees every
                 tick, which a run that recycles view slots needs (tests/track_model.py) — and the observers start at tick T
  the restored   a fresh oracle that restores the image and carries the same models from T on: its samples equal the
                 reference's, so that "a resumed run gives the same samples" is a test and not a remark

  deep(T)        tests/test_ledger.py's DEEP (512 nodes, two pages, SWIM, push-pull, all seven kinds) at T = 0 (an image with
                 nothing in flight), 1 (the first with anything in flight), 30 and 31 (queues deeper than SIM_Q_HOT, whose order in
                 the image is canonical; both buffer parities), and at 31 with the bijection fan-out
  slots(T)       tests/test_roll.py's SLOTS (4 096 nodes, 16 view slots, recycling) at T = 30 (REVIVE, CRASH, CRASH pending in the
                 image's schedule), 101 and 130 (a hole in the slots and a recycled baseline)
  ragged(n)      tests/test_observer_shapes.py's script paused where it pauses itself, at tick 10
  lazy           tests/test_lazy_planes_gpu.py's 128 Ki nodes at T = 36: the restored HIP handle maps only what the image needs
  before         observers and trackers that exist BEFORE sim_restore: the oracle side makes the same jump
  snapshots      snapshots taken and thrown away in the middle of an observed run

Everything compared is an exact integer."""
import ctypes as C
import functools

import numpy as np
import pytest

from serf_amd import _ffi
from tests import _scenario as sc
from tests import test_ledger as tl
from tests import test_observer_shapes as sh
from tests import test_roll as tr
from tests._oracle import load_oracle
from tests.census_model import CensusModel
from tests.ledger_model import LedgerModel, queued_records, wire_records
from tests.roll_model import RollModel
from tests.series_model import SeriesModel
from tests.test_lazy_planes_gpu import KW as LAZY_KW, N as LAZY_N      # (the scenarios' owners, as test_observer_shapes imports them:
from tests.test_track_gpu import FAILED, SUSPECT_OR_DEAD               # importing a GPU test module needs no GPU)
from tests.track_model import TrackModel

NEVER, NOSLOT = _ffi.TRACK_NEVER, 0xFFFFFFFF
ALIVE = 1 << _ffi.STATUS_ALIVE
STALE, ACCUSED, MISSED = _ffi.ROLL_BY_STALE, _ffi.ROLL_BY_ACCUSED, _ffi.ROLL_BY_MISSED
WINDOW = 8           # the age of the "window" tracker: registered at T with a start_tick two ticks in the past, it runs from T


class SnapHeader(C.Structure):
    """The head of the canonical image (oracle/serf_oracle.c, serf_sim_api.inc snap_header): the binding has no reader of it, and
    Case.image holds this layout to the image's own tick."""
    _fields_ = [("magic", C.c_uint32), ("abi", C.c_uint32), ("cfg", _ffi.Config), ("tick", C.c_uint64), ("n_slots", C.c_uint32),
                ("n_pending_ops", C.c_uint32), ("ops_dropped", C.c_uint64), ("slots_recycled", C.c_uint64)]


def image_header(img):
    return SnapHeader.from_buffer_copy(np.asarray(img[:C.sizeof(SnapHeader)]).tobytes())


# ---- the five models on one oracle ----
class Chain:
    """The series model steps the oracle one tick at a time; the tracker model, census, roll and ledger follow behind every
    tick, then `extra`."""

    def __init__(self, o, track=True, baselines=True):
        self.o, self.extra = o, None
        self.tm, self.cm, self.rm, self.lm = TrackModel(o) if track else None, CensusModel(o), RollModel(o), LedgerModel(o)
        if self.tm and not baselines:
            # No tracker of the case reads a baseline, so the model need not dump every view behind every tick (at 128 Ki nodes that
            # is 268 MB a tick).  tests/track_model.py has no argument for it and stays as it is — this change adds and alters no
            # model — so its two fields are set here, in the one place that needs it.
            self.tm.recycles, self.tm.prev = False, None
        self.sm = SeriesModel(o, self.behind)

    def behind(self):
        t = self.o.tick - 1
        if self.tm:
            self.tm.evaluate()
        self.cm.after_tick(t)
        self.rm.after_tick(t)
        self.lm.after_tick(t)
        if self.extra:
            self.extra()

    def start(self, plan):
        self.sm.start(*plan["series"])
        self.cm.start(*plan["census"])
        self.rm.start(*plan["roll"])
        self.lm.start(*plan["ledger"])

    def add(self, specs):
        return {name: self.tm.add(spec) for name, spec in specs} if self.tm else {}

    def step(self, k):
        self.sm.step(k)

    def reads(self):
        return dict(series=self.sm.read(), census=self.cm.read(), roll=self.rm.read(), ledger=self.lm.read(),
                    counts=dict(series=self.sm.count(), census=self.cm.count(), roll=self.rm.count(), ledger=self.lm.count()))


def plan(first, period, capacity, entries, subjects=64, top_k=8, by=STALE):
    """The four periodic observers' start arguments, in the order the library's and the models' start take them."""
    return dict(series=(first, period, capacity), census=(first, period, capacity, subjects),
                roll=(first, period, capacity, top_k, by), ledger=(list(entries), first, period, capacity))


def abi_answers(sim, asked):
    """What either library answers by itself about the state it is in: `asked` is up to 64 (kind, key, ltime)."""
    n = sim.n
    out = dict(tick=sim.tick, digest=sim.digest(), cluster_stats=sim.cluster_stats(), convergence=[sim.convergence(*r) for r in asked[:12]],
               convergence_many=sim.convergence_many(asked))
    for obs in sorted({0, n - 1}):
        st, lt = sim.members(obs)
        s = sim.stats(obs)
        out[f"members({obs})"] = (st.tolist(), lt.tolist())
        out[f"stats({obs})"] = {f: int(getattr(s, f)) for f, _ in _ffi.Stats._fields_}
    return out


def model_now(ch, setup):
    """(census_now(64), roll_now(top_k, by, nodes), ledger_now(entries)) as the models give them."""
    _, _, _, top_k, by = setup["plan"]["roll"]
    return ch.cm.now(64), ch.rm.now(top_k, by, nodes=True), ch.lm.now(setup["plan"]["ledger"][0])


def cycled(some, count=_ffi.LEDGER_MAX):
    return [some[i % len(some)] for i in range(count)]


def state_at(o):
    """The conditions of an image, measured on the oracle that is about to take it."""
    node = queued_records(o)[0]
    wk = wire_records(o)[0]
    slot_of = o.dump(_ffi.ARR_SLOTMAP).astype(np.int64)
    used = np.sort(slot_of[slot_of != NOSLOT])
    return dict(deepest=int(np.bincount(node).max()) if len(node) else 0, queued=len(node), in_flight=len(wk),
                kinds_in_flight=sorted(set(wk.tolist())), slots=used.tolist(), hole=len(used) > 0 and used.tolist() != list(range(len(used))),
                slots_recycled=o.cluster_stats()["slots_recycled"])


class Case:
    def __init__(self, what, n, kw, T, ticks, before, at, after=None, answers=None, watch=None, baselines=True):
        self.what, self.n, self.kw, self.T, self.ticks, self.before, self.at, self.watch = what, n, kw, T, ticks, before, at, watch
        self.recycles = bool(kw.get("recycle_interval"))     # the tracker model then has to see the run from tick 0
        self.baselines = baselines                           # False: no tracker of the case is about a member
        self.after = after or (lambda sim, step, setup: step(ticks - T))
        self.answers = answers or (lambda sim, setup: abi_answers(sim, setup["asked"]))

    def make(self):
        return _ffi.Sim(load_oracle(), _ffi.make_config(self.n, **self.kw))

    def image(self):
        """(the image at tick T, its conditions), from an oracle of its own."""
        a = self.make()
        self.before(a)
        if self.T:
            a.step(self.T)
        cond = state_at(a)
        img = a.snapshot()
        a.close()
        hd = image_header(img)
        assert hd.tick == self.T and len(cond["slots"]) <= hd.n_slots
        cond.update(n_slots=int(hd.n_slots), pending_ops=int(hd.n_pending_ops), bytes=len(img))
        return img, cond

    def carry(self, o, ch, setup, look=()):
        """From tick T to the end on an oracle with the models chained; `look`: ticks behind which model_now is taken as well."""
        ch.start(setup["plan"])
        handles = ch.add(setup["specs"])
        now = {self.T: (abi_answers(o, setup["asked"]), model_now(ch, setup))}

        def extra():
            if o.tick in look:
                now[o.tick] = (abi_answers(o, setup["asked"]), model_now(ch, setup))
        ch.extra = extra
        self.after(o, ch.step, setup)
        ch.extra = None
        assert o.tick == self.ticks
        return dict(reads=ch.reads(), trackers={k: ch.tm.result(h) for k, h in handles.items()}, now=now, end=self.answers(o, setup),
                    bounds=o.cluster_stats())

    def reference(self, look=None):
        """The uninterrupted oracle: models chained from tick 0, observers started at T.  watch(o), when the case has one, runs
        behind every tick up to T; what it returned goes to at()."""
        o = self.make()
        self.before(o)
        ch = Chain(o, baselines=self.baselines)
        seen = []
        if self.watch:
            ch.extra = lambda: seen.append(self.watch(o))
        ch.step(self.T)
        ch.extra = None
        setup = self.at(o, ch, seen)
        out = self.carry(o, ch, setup, (self.T + 1,) if look is None else look)
        out.update(setup=setup, o=o)
        return out

    def restored(self, img, setup, look=()):
        """A fresh oracle that restores the image and carries the same models from T on — without the tracker model where the
        run recycles view slots: it cannot learn a recycled baseline on an oracle it did not see from tick 0."""
        b = self.make()
        b.restore(img)
        assert b.tick == self.T
        out = self.carry(b, Chain(b, track=not self.recycles), setup, look)
        b.close()
        return out


def same_words(a, b):
    if isinstance(a, (tuple, list)) and len(a) and isinstance(a[0], (np.ndarray, np.void)):
        return len(a) == len(b) and all(same_words(x, y) for x, y in zip(a, b))
    if isinstance(a, (np.ndarray, np.void)):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def assert_same_run(got, want, what):
    """Two oracle runs with the models chained, word for word (the trackers where the restored side has a tracker model)."""
    for k, w in want["reads"].items():
        assert same_words(got["reads"][k], w), f"{what}: {k} differs"
    if got["trackers"]:
        assert got["trackers"] == want["trackers"], what
    for t, (abi, models) in got["now"].items():
        wabi, wmodels = want["now"][t]
        for k in wabi:
            assert abi[k] == wabi[k], f"{what}: {k} at tick {t}: {abi[k]} != {wabi[k]}"
        for g, w, name in zip(models, wmodels, ("census_now", "roll_now", "ledger_now")):
            assert same_words(g, w), f"{what}: {name} at tick {t}"
    assert got["end"] == want["end"], what


def inside_bounds(run):
    assert run["bounds"]["overflow"] == 0 and run["bounds"]["ops_dropped"] == 0       # the run stays inside the model's bounds


def due(T, ticks, first, period):
    """The ticks whose samples a sampler holds that was started with (first, period) before or at T on a handle that is at T."""
    return [t + 1 for t in range(T, ticks) if t >= first and (t - first) % period == 0]


# ---- deep ----
DEEP_FANS = dict(krandomnodes=tl.DEEP_KW, bijection=dict(tl.DEEP_KW, flags=_ffi.CF_BASELINE_JOINED))
DEEP_EVEN, DEEP_ODD = 30, 31
PASSED_FIRST, PASSED_PERIOD = 2, 4         # a sampler started at DEEP_ODD with a first tick that has passed: T, T + 4, ... and not 2 + 4 i
DEEP_CASES = [("krandomnodes", 0), ("krandomnodes", 1), ("krandomnodes", DEEP_EVEN), ("krandomnodes", DEEP_ODD), ("bijection", DEEP_ODD)]
DEEP_OPS = sc.schedule(tl.DEEP_N, 40, rate=2.0, seed=524, max_member_subjects=40)        # tl.deep_drive's


@functools.lru_cache(maxsize=None)
def deep_entries(fan):
    """(the 64 entries dealt from a dry run, 64 rumours for sim_convergence_many: the entries' first, then others that occur)."""
    if fan == "krandomnodes":
        _, entries, _, _, _, found = tl.deep_oracle()
    else:
        found, _ = tl.dry_run(tl.maker(tl.DEEP_N, DEEP_FANS[fan]), tl.deep_drive, tl.EVERY)
        entries = tl.deal(found)
    rumours = [e for e in entries if e[0] <= _ffi.K_QUERY]
    rumours += [e for e in sorted(found) if e[0] <= _ffi.K_QUERY and e not in rumours]
    assert len(entries) == _ffi.LEDGER_MAX and len(rumours) >= _ffi.LEDGER_MAX
    return entries, rumours[:_ffi.LEDGER_MAX]


def deep_victim(T):
    """The first node the schedule crashes after T without having it leave first."""
    leavers = {op[2] for op in DEEP_OPS if op[1] == _ffi.OP_LEAVE}
    later = [op for op in DEEP_OPS if op[1] == _ffi.OP_CRASH and op[0] > T and op[2] not in leavers]
    assert later, f"the schedule crashes nobody after tick {T}"
    return later[0][2], later[0][0]


def deep_specs(ch, entries, T):
    """A JOIN, a LEAVE, an EVENT and a QUERY identity of the entries — of each kind the one with the most queued copies at T, the
    first when none is queued — and three MEMBER trackers about the node that crashes next."""
    _, rec = ch.lm.now(entries)
    specs = []
    for kind, name in ((_ffi.K_JOIN, "join"), (_ffi.K_LEAVE, "leave"), (_ffi.K_EVENT, "event"), (_ffi.K_QUERY, "query")):
        cols = [i for i, e in enumerate(entries) if e[0] == kind]
        best = max(cols, key=lambda i: (int(rec["queued"][i]), -i))
        specs.append((name, _ffi.rumour_tracker(*entries[best])))
    victim, _ = deep_victim(T)
    specs += [("suspicion", _ffi.member_tracker(victim, FAILED, SUSPECT_OR_DEAD)), ("failed", _ffi.member_tracker(victim, FAILED)),
              ("window", _ffi.member_tracker(victim, FAILED, start=max(T - 2, 0), max_age=WINDOW))]
    return specs


def deep_case(fan, T, passed=False):
    entries, asked = deep_entries(fan)

    def at(o, ch, seen):
        # passed: a first tick that has passed means "now", which is T on a restored handle — with a period that shows the difference
        first, period = (PASSED_FIRST, PASSED_PERIOD) if passed else (T, 1)
        return dict(plan=plan(first, period, tl.DEEP_TICKS, entries), specs=deep_specs(ch, entries, T), asked=asked)
    return Case(f"deep({T}) {fan}" + (" passed" if passed else ""), tl.DEEP_N, DEEP_FANS[fan], T, tl.DEEP_TICKS,
                lambda sim: sc.apply_schedule(sim, DEEP_OPS), at)


@functools.lru_cache(maxsize=None)
def deep_run(fan, T, passed=False):
    """Once per session; nobody changes what it returns: (case, image, its conditions, the reference run)."""
    case = deep_case(fan, T, passed)
    img, cond = case.image()
    return case, img, cond, case.reference(look=(T + 1, 18))      # (tick 18: test_snapshots_* looks there)


def check_deep(fan, T, cond, ref):
    inside_bounds(ref)
    if T == 0:
        assert cond["in_flight"] == 0 and cond["queued"] == 0 and cond["pending_ops"] == len(DEEP_OPS)
    elif T == 1:
        assert cond["in_flight"] > 0
    else:
        assert cond["deepest"] > _ffi.Q_HOT, "no queue deeper than SIM_Q_HOT at T"
        assert len(cond["kinds_in_flight"]) >= 5 and cond["in_flight"] > 10000
        if fan == "krandomnodes":
            assert tl.deep_oracle()[3][T - 1][3] == cond["deepest"]                      # deep_probe behind tick T - 1
    trk = ref["trackers"]
    assert len(trk) == 7 and deep_victim(T)[1] > T
    assert trk["suspicion"]["first"] != NEVER and trk["suspicion"]["first"] > deep_victim(T)[1]
    # the window runs from T, not from its start_tick: WINDOW evaluations, none of which latches `all`
    assert (trk["window"]["evaluated"], trk["window"]["all"], trk["window"]["state"]) == (WINDOW, NEVER, 2)
    if T >= DEEP_EVEN:
        assert any(0 < trk[k]["last"] for k in ("join", "leave", "event", "query"))
    hdr, rec = ref["reads"]["ledger"]
    assert hdr["tick"].tolist() == list(range(T + 1, tl.DEEP_TICKS + 1)) and rec["queued"].max() > 0 and rec["in_flight"].max() > 0


@pytest.mark.parametrize("fan,T", DEEP_CASES)
def test_deep_resumed_on_the_oracle(fan, T):
    case, img, cond, ref = deep_run(fan, T)
    check_deep(fan, T, cond, ref)
    assert_same_run(case.restored(img, ref["setup"], look=(T + 1,)), ref, case.what)


def check_passed(T, ref):
    want = due(T, tl.DEEP_TICKS, T, PASSED_PERIOD)
    assert len(want) > 5 and want[0] == T + 1 and (T - PASSED_FIRST) % PASSED_PERIOD     # (sampling by the first tick as given would differ)
    assert ref["reads"]["series"][:, 0].tolist() == ref["reads"]["census"][0]["tick"].tolist() == want
    assert ref["reads"]["roll"][0]["tick"].tolist() == ref["reads"]["ledger"][0]["tick"].tolist() == want


def test_a_first_tick_that_has_passed_is_the_restored_tick_on_the_oracle():
    case, img, cond, ref = deep_run("krandomnodes", DEEP_ODD, True)
    check_passed(DEEP_ODD, ref)
    assert_same_run(case.restored(img, ref["setup"], look=(DEEP_ODD + 1,)), ref, case.what)


# ---- slots ----
SLOTS_T = {30: STALE, 101: ACCUSED, 130: MISSED}               # T -> the roll's rank_by
SLOTS_NEVER = tr.N // 2                                         # a subject that never gets a view slot
SLOTS_NEXT = {30: 2000, 101: 7, 130: 7}                        # the subject the cluster is about to, or busy to, declare failed


def slots_before(sim):
    tr.slots_script(sim, lambda k: None)


@functools.lru_cache(maxsize=None)
def slots_found():
    """{tick: identities queued at a running node or in flight behind tick - 1}, from a run of its own."""
    o = _ffi.Sim(load_oracle(), _ffi.make_config(tr.N, **tr.SLOTS_KW))
    slots_before(o)
    out = {}
    for _ in range(tr.SLOTS_TICKS):
        o.step(1)
        _, kind, key, val, _, _ = queued_records(o)
        wk, wkey, wval, _ = wire_records(o)
        out[o.tick] = set(zip(kind.tolist(), key.tolist(), val.tolist())) | set(zip(wk.tolist(), wkey.tolist(), wval.tolist()))
    o.close()
    return out


def slots_case(T):
    def watch(o):
        return set(np.nonzero(o.dump(_ffi.ARR_SLOTMAP) != NOSLOT)[0].tolist())

    def at(o, ch, seen):
        had = set().union(*seen) if seen else set()
        gone = sorted(had - seen[-1])                                                    # had a slot earlier, has none at T
        nxt, v = SLOTS_NEXT[T], SLOTS_NEVER
        lt100 = int(o.members(0)[1][100])
        specs = [("never alive", _ffi.member_tracker(v, ALIVE)), ("never join", _ffi.rumour_tracker(_ffi.K_JOIN, v, 1)),
                 ("never leave", _ffi.rumour_tracker(_ffi.K_LEAVE, v, 2)), ("suspicion", _ffi.member_tracker(nxt, FAILED, SUSPECT_OR_DEAD)),
                 ("failed", _ffi.member_tracker(nxt, FAILED)), ("window", _ffi.member_tracker(nxt, FAILED, start=T - 2, max_age=WINDOW))]
        asked = [(k, v, t) for k in (_ffi.K_JOIN, _ffi.K_LEAVE) for t in (1, 2)] + [(_ffi.K_JOIN, nxt, 1), (_ffi.K_LEAVE, 100, lt100)]
        base = None
        if gone:
            r = gone[0]
            lt, inc, bits = base = ch.tm.base[r]                                         # the baseline the recycling pass left
            specs += [("recycled alive", _ffi.member_tracker(r, ALIVE, min_inc=inc)), ("recycled newer", _ffi.member_tracker(r, ALIVE, min_inc=inc + 1)),
                      ("recycled join", _ffi.rumour_tracker(_ffi.K_JOIN, r, lt)), ("recycled join + 1", _ffi.rumour_tracker(_ffi.K_JOIN, r, lt + 1))]
            asked += [(k, r, t) for k in (_ffi.K_JOIN, _ffi.K_LEAVE) for t in (lt, lt + 1)]
        # four identities that are carried at T or later; when the run has fewer left, identities of the script's subjects
        found = set().union(*(ids for t, ids in slots_found().items() if t >= max(T, 1)))
        entries = tl.deal(found, 3)
        entries += [e for e in ((_ffi.K_LEAVE, 100, lt100), (_ffi.K_JOIN, 300, 1), (_ffi.K_DEAD, 7, 0), (_ffi.K_ALIVE, 300, 1)) if e not in entries]
        return dict(plan=plan(T, 1, tr.SLOTS_TICKS, entries[:4], 64, tr.TOP_K, SLOTS_T[T]), specs=specs, asked=cycled(asked), gone=gone,
                    base=base, had=had)
    return Case(f"slots({T})", tr.N, tr.SLOTS_KW, T, tr.SLOTS_TICKS, slots_before, at, watch=watch)


@functools.lru_cache(maxsize=None)
def slots_run(T):
    case = slots_case(T)
    img, cond = case.image()
    return case, img, cond, case.reference()


def check_slots(T, cond, ref):
    inside_bounds(ref)
    setup, trk = ref["setup"], ref["trackers"]
    up = ref["end"]["cluster_stats"]["up"]
    assert SLOTS_NEVER not in setup["had"] and ref["o"].dump(_ffi.ARR_SLOTMAP)[SLOTS_NEVER] == NOSLOT
    assert trk["never alive"]["all"] == T + 1 and trk["never join"]["all"] == T + 1 and trk["never leave"]["last"] == 0
    assert (trk["window"]["evaluated"], trk["window"]["all"]) == (WINDOW, NEVER)
    if T == 30:
        assert cond["pending_ops"] >= 3 and not cond["hole"] and cond["slots_recycled"] == 0 and not setup["gone"]
        assert trk["suspicion"]["first"] > 50
    else:
        assert cond["hole"] and cond["slots_recycled"] > 0, "the image was to carry a free slot below an allocated one"
        assert setup["gone"] == [300] and setup["base"] != (1, 0, 3), "a recycled baseline that is not the creation baseline"
        lt, inc, _ = setup["base"]
        assert trk["recycled alive"]["all"] == T + 1 and trk["recycled join"]["all"] == T + 1
        assert trk["recycled newer"]["peak"] == 0 and trk["recycled join + 1"]["peak"] == 0
        asked = setup["asked"]
        i = asked.index((_ffi.K_JOIN, 300, lt))
        for t, (abi, _) in ref["now"].items():
            assert abi["convergence_many"][0][i] == abi["cluster_stats"]["up"] and abi["convergence_many"][0][i + 1] == 0
        assert trk["suspicion"]["peak"] > 0
    hdr, rec = ref["reads"]["ledger"]
    assert rec.shape == (tr.SLOTS_TICKS - T, 4) and rec["queued"].max() > 0 and rec["reach"].max() >= up - 2
    assert (ref["reads"]["roll"][0]["listed"] >> 32 == SLOTS_T[T]).all()


@pytest.mark.parametrize("T", sorted(SLOTS_T))
def test_slots_resumed_on_the_oracle(T):
    case, img, cond, ref = slots_run(T)
    check_slots(T, cond, ref)
    assert_same_run(case.restored(img, ref["setup"], look=(T + 1,)), ref, case.what)


# ---- ragged ----
RESUME_SIZES = (1, 3, 65, 257, 1025)
RAGGED_T = 10
# (sh.ragged_kw and its seed table unchanged: under these seeds every tracker that starts at tick 10 still latches `all` within the
# 90 ticks, which check_ragged asserts — a size for which it did not would get a seed of its own here, the way sh.RAGGED_SEED does it)


def ragged_case(n, fan):
    """sh.ragged_script cut where it pauses: `before` is its part up to step(10), `after` the rest; all six trackers are
    registered at tick 10 (test_ragged_is_the_script_of_the_shapes holds the two halves to the whole)."""
    last = n - 1

    def before(sim):
        if n > 1:
            sim.inject(4, _ffi.OP_CRASH, last)
        sim.user_event(0, sh.EVENT_KEY, 64)

    def at(o, ch, seen):
        ru = dict(event=(_ffi.K_EVENT, sh.EVENT_KEY, 1), join=(_ffi.K_JOIN, last, 1))
        specs = []
        if n > 1:
            specs += [("suspicion", _ffi.member_tracker(last, FAILED, SUSPECT_OR_DEAD, start=4)), ("failed", _ffi.member_tracker(last, FAILED, start=4)),
                      ("window", _ffi.member_tracker(last, FAILED, start=4, max_age=WINDOW))]
        if n > 2:
            ru["leave"] = (_ffi.K_LEAVE, n - 2, o.stats(n - 2).member_time)
        ru["query"] = (_ffi.K_QUERY, sh.QUERY_ID, o.stats(0).query_time)
        specs += [(k, _ffi.rumour_tracker(*ru[k])) for k in ("event", "join", "leave", "query") if k in ru]
        entries = list(ru.values()) + [(_ffi.K_ALIVE, 0, 0)] + ([(_ffi.K_SUSPECT, last, 0), (_ffi.K_DEAD, last, 0)] if n > 1 else [])
        noslot = None
        if sh.ragged_kw(n, fan)["view_slots"]:
            noslot = sh.ragged_oracle(n, fan)["noslot"]
        return dict(plan=plan(RAGGED_T, 1, sh.RAGGED_TICKS, entries, sh.CENSUS_SUBJECTS), specs=specs, asked=sh.five_rumours(ru, n), ru=ru, noslot=noslot)

    def after(sim, step, setup):
        if n > 2:
            sim.leave(n - 2)
        sim.query(0, sh.QUERY_ID, _ffi.F_ACK)
        step(sh.RAGGED_TICKS - RAGGED_T)

    def answers(sim, setup):
        return sh.answers(sim, n, setup["ru"], setup["noslot"])
    return Case(f"ragged({n}) {fan}", n, sh.ragged_kw(n, fan), RAGGED_T, sh.RAGGED_TICKS, before, at, after, answers)


@functools.lru_cache(maxsize=None)
def ragged_run(n, fan):
    case = ragged_case(n, fan)
    img, cond = case.image()
    return case, img, cond, case.reference(look=())


def check_ragged(n, fan, cond, ref):
    inside_bounds(ref)
    trk, setup = ref["trackers"], ref["setup"]
    assert len(trk) == (7 if n > 2 else 3)
    if n >= 3:
        for name, r in trk.items():
            if name != "window":
                assert r["all"] != NEVER and r["all"] < sh.RAGGED_TICKS and r["state"] == 2, (name, r)
    if n >= 65:
        assert (trk["window"]["evaluated"], trk["window"]["all"]) == (WINDOW, NEVER)     # ticks 10 .. 17, not 4 .. 11
    if n <= 3:
        assert n - 1 < sh.KW["fanout"]          # fewer other nodes than the fan-out: cells without a target, feff below the fan-out
    assert ref["reads"]["series"].shape == (sh.RAGGED_TICKS - RAGGED_T, 64)
    assert setup["ru"] == sh.ragged_oracle(n, fan)["rumours"]
    assert ref["end"]["digest"] == sh.ragged_oracle(n, fan)["answers"]["digest"], "the two halves are not the script"
    assert ref["end"]["cluster_stats"] == sh.ragged_oracle(n, fan)["answers"]["cluster_stats"]


@pytest.mark.parametrize("fan", sorted(sh.FANOUTS))
@pytest.mark.parametrize("n", RESUME_SIZES)
def test_ragged_resumed_on_the_oracle(n, fan):
    case, img, cond, ref = ragged_run(n, fan)
    check_ragged(n, fan, cond, ref)
    assert_same_run(case.restored(img, ref["setup"]), ref, case.what)


# ---- lazy planes ----
# (20 ticks after T: behind tick 56 the first queue of this schedule overflows, and a run beyond the model's bounds is no reference)
LAZY_T, LAZY_AFTER, LAZY_PERIOD, LAZY_SAMPLES = 36, 20, 8, 3
LAZY_KEY, LAZY_AHEAD = 0x5000, 10            # an event nobody sent, at a Lamport time this far beyond every clock in the image
LAZY_FLAGS = _ffi.CF_BASELINE_JOINED | _ffi.CF_RANDOM_FANOUT


def lazy_case():
    def before(sim):
        for op in sc.schedule(LAZY_N, 40, rate=0.6, seed=5, max_member_subjects=20):
            sim.inject(*op)

    def at(o, ch, seen):
        rows = o.dump(_ffi.ARR_ROWS)
        ahead = (_ffi.K_EVENT, LAZY_KEY, int(rows["event_clock"].max()) + LAZY_AHEAD)
        _, kind, key, val, _, _ = queued_records(o)
        live = sorted(set(zip(kind.tolist(), key.tolist(), val.tolist())))
        entries = [next(e for e in live if e[0] == _ffi.K_LEAVE), next(e for e in live if e[0] == _ffi.K_EVENT), ahead]
        # census, roll, ledger and series with a first tick that has passed: behind ticks 36, 44 and 52
        return dict(plan=plan(0, LAZY_PERIOD, LAZY_SAMPLES, entries), specs=[("ahead", _ffi.rumour_tracker(*ahead))], asked=entries,
                    clocks=(int(rows["event_clock"].max()), int(rows["query_clock"].max())))
    return Case("lazy", LAZY_N, dict(LAZY_KW, flags=LAZY_FLAGS), LAZY_T, LAZY_T + LAZY_AFTER, before, at, baselines=False)


@functools.lru_cache(maxsize=None)
def lazy_reference():
    """The reference run without its oracle (the handles of this size are closed as soon as they have answered)."""
    ref = lazy_case().reference(look=())
    ref.pop("o").close()
    return ref


def check_lazy(cond, ref):
    inside_bounds(ref)
    setup = ref["setup"]
    assert 0 < cond["n_slots"] < LAZY_KW["view_slots"] and cond["in_flight"] > 0
    assert setup["clocks"][0] + LAZY_AHEAD + 2 < LAZY_KW["event_ring"], "the identity's plane lies beyond what the restore maps"
    hdr, rec = ref["reads"]["ledger"]
    assert hdr["tick"].tolist() == [LAZY_T + 1 + LAZY_PERIOD * i for i in range(LAZY_SAMPLES)] == ref["reads"]["census"][0]["tick"].tolist()
    assert rec["queued"][:, :2].max() > 0 and rec["reach"][:, :2].max() > 0
    row = rec[:, 2]                                                                      # nobody holds it: the identity and zeros
    assert (row["id"] == (LAZY_KEY | _ffi.K_EVENT << 32)).all() and (row["val"] == setup["asked"][2][2]).all()
    assert not any(row[f].any() for f in ("reach", "holders", "queued", "transmits", "in_flight", "fresh"))
    assert ref["trackers"]["ahead"]["evaluated"] == LAZY_AFTER and ref["trackers"]["ahead"]["peak"] == 0


def test_lazy_resumed_on_the_oracle():
    case = lazy_case()
    ref = lazy_reference()
    img, cond = case.image()
    check_lazy(cond, ref)
    got = case.restored(img, ref["setup"])
    del img
    assert_same_run(got, ref, case.what)


# ---- observers that exist before sim_restore ----
BEFORE_T = DEEP_ODD
BEFORE_CENSUS_CAPACITY = 30                  # of the 41 samples due: `dropped` counts


def before_plan(entries):
    T = BEFORE_T
    return dict(series=(3, 4, tl.DEEP_TICKS), census=(0, 1, BEFORE_CENSUS_CAPACITY, 64), roll=(T + 5, 1, tl.DEEP_TICKS, 8, STALE),
                ledger=(list(entries), 0, 3, tl.DEEP_TICKS))


def before_specs(entries):
    """Windows fixed at registration, at tick 0, in absolute ticks: one the restore jumps over, one that straddles T, one
    that opens after T, and a tracker without an age."""
    T, (victim, _) = BEFORE_T, deep_victim(BEFORE_T)
    event = next(e for e in reversed(entries) if e[0] == _ffi.K_EVENT)
    spreading = dict(deep_run("krandomnodes", T)[3]["setup"]["specs"])["event"]           # the event with the most queued copies at T
    spreading = (spreading.a, spreading.b, spreading.ltime)
    return [("jumped", _ffi.rumour_tracker(*event, start=0, max_age=4)), ("straddles", _ffi.member_tracker(victim, FAILED, start=T - 2, max_age=8)),
            ("opens later", _ffi.rumour_tracker(*spreading, start=T + 5, max_age=4)), ("no age", _ffi.rumour_tracker(*event))]


@functools.lru_cache(maxsize=None)
def before_reference():
    """A fresh oracle treated as the HIP handle is: models started and trackers added at tick 0, restore, step to the end."""
    entries, asked = deep_entries("krandomnodes")
    _, img, _, _ = deep_run("krandomnodes", BEFORE_T)
    o = _ffi.Sim(load_oracle(), _ffi.make_config(tl.DEEP_N, **tl.DEEP_KW))
    ch = Chain(o)
    ch.start(before_plan(entries))
    handles = ch.add(before_specs(entries))
    o.restore(img)
    ch.step(tl.DEEP_TICKS - BEFORE_T)
    return dict(o=o, reads=ch.reads(), trackers={k: ch.tm.result(h) for k, h in handles.items()}, end=abi_answers(o, asked), bounds=o.cluster_stats())


def check_before(ref):
    inside_bounds(ref)
    T, ticks, reads, trk = BEFORE_T, tl.DEEP_TICKS, ref["reads"], ref["trackers"]
    assert reads["series"][:, 0].tolist() == due(T, ticks, 3, 4) and (T - 3) % 4 == 0
    assert reads["census"][0]["tick"].tolist() == due(T, ticks, 0, 1)[:BEFORE_CENSUS_CAPACITY]
    assert reads["counts"]["census"] == (BEFORE_CENSUS_CAPACITY, ticks - T - BEFORE_CENSUS_CAPACITY)
    assert reads["roll"][0]["tick"].tolist() == due(T, ticks, T + 5, 1) and reads["ledger"][0]["tick"].tolist() == due(T, ticks, 0, 3)
    never = {k: NEVER for k in ("first", "half", "p90", "p99", "all")}
    assert trk["jumped"] == dict(never, evaluated=0, peak=0, last=0, last_up=0, state=0)
    assert (trk["straddles"]["evaluated"], trk["straddles"]["all"], trk["straddles"]["state"]) == (6, NEVER, 2)
    assert trk["opens later"]["evaluated"] == 4 and trk["opens later"]["state"] == 2 and 0 < trk["opens later"]["last"] < trk["opens later"]["last_up"]
    assert trk["no age"]["evaluated"] > 0 and trk["no age"]["peak"] > 0
    assert ref["end"]["digest"] == deep_run("krandomnodes", T)[3]["end"]["digest"]


def test_observers_before_a_restore_on_the_oracle():
    check_before(before_reference())


# ---- snapshots in the middle of an observed run ----
SNAPSHOTS_AT = (17, 18, 40)
CENSUS_NOW_AT = 18


def snapshots_script(sim, step, census_now):
    """DEEP from tick 0 in stretches, an image taken and thrown away between them; returns what census_now() gave at tick 18."""
    seen = None
    for t in SNAPSHOTS_AT + (tl.DEEP_TICKS,):
        step(t - sim.tick)
        if t in SNAPSHOTS_AT:
            sim.snapshot()
        if t == CENSUS_NOW_AT:
            seen = census_now()
    return seen


def test_snapshots_do_not_disturb_the_models_on_the_oracle():
    """The reference of tests/test_observer_resume_gpu.py's test of that name is deep_run(0), which takes no snapshot; an oracle
    that takes them gives the same samples."""
    case, _, _, ref = deep_run("krandomnodes", 0)
    o = case.make()
    case.before(o)
    ch = Chain(o)
    ch.start(ref["setup"]["plan"])
    handles = ch.add(ref["setup"]["specs"])
    seen = snapshots_script(o, ch.step, lambda: ch.cm.now(64))
    assert same_words(seen, ref["now"][CENSUS_NOW_AT][1][0])
    for k, w in ref["reads"].items():
        assert same_words(ch.reads()[k], w), k
    assert {k: ch.tm.result(h) for k, h in handles.items()} == ref["trackers"] and o.digest() == ref["end"]["digest"]
    o.close()
