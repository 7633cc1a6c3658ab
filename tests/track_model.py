"""Reference model of the device-resident trackers (include/serf_sim_track.h).

Steps any ``_ffi.Sim`` — in the tests: the CPU oracle — ONE tick at a time and evaluates the header's definitions with
numpy after every tick:

* MEMBER trackers and JOIN / LEAVE rumours from ``dump(ARR_ROWS / ARR_VIEW / ARR_SLOTMAP)``;
* EVENT / QUERY rumours from the library's own ``convergence_many`` (the rings' overflow rows are its business).

A subject WITHOUT a view slot sits at its baseline, which no dump shows.  It is the creation baseline
(``CF_BASELINE_JOINED``: known, Alive, ltime 1, incarnation 0, memberlist alive; otherwise all zero) until the subject's
slot is recycled, and from then on the entry the running nodes agreed on: the recycling pass runs first in its tick and
frees a slot only when every running node holds the same entry of it, so the model carries forward the entry a running
observer held in the dump of the tick before the slot disappeared, and cross-checks status and ltime with
``members(observer)``.  For that the model has to see every tick of a run that recycles: create it at tick 0 and step
the simulator through ``TrackModel.step`` only.
"""
import numpy as np

from serf_amd import _ffi

NOSLOT = 0xFFFFFFFF
NEVER = _ffi.TRACK_NEVER
FIELDS = ("first", "half", "p90", "p99", "all", "evaluated", "peak", "last", "last_up", "state")


def new_result():
    r = dict.fromkeys(FIELDS, 0)
    for k in ("first", "half", "p90", "p99", "all"):
        r[k] = NEVER
    return r


def latch(r, count, up, now, last_tick_of_window):
    """One evaluation (integer arithmetic throughout)."""
    count, up = int(count), int(up)
    r["evaluated"] += 1
    r["last"], r["last_up"] = count, up
    r["peak"] = max(r["peak"], count)
    if up > 0:
        for name, ok in (("first", count >= 1), ("half", 2 * count >= up), ("p90", 10 * count >= 9 * up),
                         ("p99", 100 * count >= 99 * up), ("all", count == up)):
            if ok and r[name] == NEVER:
                r[name] = now
    r["state"] = 2 if (r["all"] != NEVER or last_tick_of_window) else 1


class TrackModel:
    def __init__(self, sim):
        self.sim, self.n = sim, sim.n
        self.trk = {}          # handle -> dict(spec, start, end, res)
        self.next = 0
        joined = bool(sim.cfg.flags & _ffi.CF_BASELINE_JOINED)
        self.base0 = (1, 0, 1 | (_ffi.STATUS_ALIVE << 1)) if joined else (0, 0, 0)   # (ltime, inc, bits)
        self.base = {}         # subject -> (ltime, inc, bits) after a recycling pass freed its slot
        self.recycles = bool(sim.cfg.recycle_interval)
        self.prev = None       # (slot map, view [A][N], up) of the tick before
        if self.recycles:
            assert sim.tick == 0, "a run that recycles view slots has to be modelled from its first tick"
            self.prev = self._dumps()

    # ---- registration: same arguments as the library's ----
    def add(self, spec):
        """spec: _ffi.Tracker.  Returns the model's handle of the tracker."""
        start = max(int(spec.start_tick), self.sim.tick)
        end = start + int(spec.max_age) if spec.max_age else 0
        if end > 0xFFFFFFFF:
            end = 0
        k = self.next
        self.next += 1
        self.trk[k] = dict(spec=_ffi.Tracker(spec.kind, spec.a, spec.b, spec.min_inc, spec.ltime, spec.start_tick, spec.max_age),
                           start=start, end=end, res=new_result())
        return k

    def remove(self, k):
        del self.trk[k]

    def result(self, k):
        return dict(self.trk[k]["res"])

    # ---- stepping ----
    def step(self, n=1):
        for _ in range(n):
            self.sim.step(1)
            self.evaluate()

    def _dumps(self):
        s = self.sim
        rows = s.dump(_ffi.ARR_ROWS)
        up = (rows["flags"] & 1).astype(bool)
        slot = s.dump(_ffi.ARR_SLOTMAP).copy()
        view = s.dump(_ffi.ARR_VIEW)
        view = view.reshape(view.size // self.n, self.n)
        return slot, view, up

    def _entry(self, subject, slot, view):
        """(ltime, inc, bits) of every node's entry of `subject`: arrays [N], or scalars for a slot-less subject."""
        a = int(slot[subject])
        if a != NOSLOT:
            e = view[a]
            return e["ltime"], e["inc"], e["bits"]
        lt, inc, bits = self.base.get(subject, self.base0)
        return np.uint64(lt), np.uint32(inc), np.uint32(bits)

    def _note_recycled(self, slot, up):
        pslot, pview, pup = self.prev
        gone = np.nonzero((pslot != NOSLOT) & (slot == NOSLOT))[0]
        if not gone.size:
            return
        assert pup.any()
        obs = int(np.argmax(pup))   # a node that was running when the pass ran
        st = lt = None
        if up[obs]:
            st, lt = self.sim.members(obs)
        for x in gone.tolist():
            e = pview[int(pslot[x])][obs]
            self.base[x] = (int(e["ltime"]), int(e["inc"]), int(e["bits"]))
            if st is not None:   # what the library reads for the slot-less subject now
                known = int(e["bits"]) & 1
                assert int(st[x]) == (((int(e["bits"]) >> 1) & 7) if known else 0), f"subject {x}: baseline status"
                assert int(lt[x]) == (int(e["ltime"]) if known else 0), f"subject {x}: baseline ltime"

    def count_view(self, spec, slot, view, up):
        subject = spec.a if spec.kind == _ffi.TRK_MEMBER else spec.b
        lt, inc, bits = self._entry(subject, slot, view)
        known = (bits & 1).astype(bool)
        if spec.kind == _ffi.TRK_MEMBER:
            smask, wmask = np.uint32(spec.b & 0xFF), np.uint32(spec.b >> 8)
            st = np.where(known, (bits >> np.uint32(1)) & np.uint32(7), np.uint32(0)).astype(np.uint32)
            sw = ((bits >> np.uint32(4)) & np.uint32(3)).astype(np.uint32)
            hit = (((smask >> st) & 1).astype(bool) | (known & ((wmask >> sw) & 1).astype(bool))) & (inc >= np.uint32(spec.min_inc))
        else:
            hit = known & (lt >= np.uint64(spec.ltime))
        return int((np.broadcast_to(hit, up.shape) & up).sum())

    def evaluate(self):
        """After a tick: sim.tick is the value the latches take."""
        s = self.sim
        now = s.tick
        t = now - 1
        act = [v for v in self.trk.values() if v["res"]["state"] != 2 and v["start"] <= t and (not v["end"] or t < v["end"])]
        view_kind = [v for v in act if v["spec"].kind == _ffi.TRK_MEMBER or v["spec"].a in (_ffi.K_JOIN, _ffi.K_LEAVE)]
        ring_kind = [v for v in act if v not in view_kind]
        if self.recycles or view_kind:
            slot, view, up = self._dumps()
            if self.recycles:
                self._note_recycled(slot, up)
                self.prev = (slot, view.copy(), up)
            nup = int(up.sum())
            for v in view_kind:
                latch(v["res"], self.count_view(v["spec"], slot, view, up), nup, now, v["end"] == now)
        for j in range(0, len(ring_kind), 64):
            part = ring_kind[j:j + 64]
            seen, nup = s.convergence_many([(v["spec"].a, v["spec"].b, v["spec"].ltime) for v in part])
            for v, c in zip(part, seen):
                latch(v["res"], c, nup, now, v["end"] == now)
