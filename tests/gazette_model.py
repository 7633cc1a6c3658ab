"""Reference model of the member gazette (include/serf_sim_gazette.h): the samples and both maps computed with numpy from the
canonical dumps (ARR_VIEW / ARR_SLOTMAP / ARR_ROWS) of any _ffi.Sim that is stepped one tick at a time, whatever the period —
the model keeps every subject's baseline itself: what sim_create sets (known / Alive when the cluster starts joined, otherwise
zero), and afterwards the entry the running nodes held in the last dump before the subject lost its slot.  The CPU oracle has
no gazette; with this model it is the checker of the HIP library's."""
import numpy as np

from serf_amd import _ffi
from tests.census_model import NOSLOT, RF_UP, subjects

WORDS, COLS = _ffi.GAZETTE_WORDS, _ffi.GAZETTE_COLS
STAMP_MASK = 0x1FFFFF
ALIVE, LEFT, FAILED = _ffi.STATUS_ALIVE, _ffi.STATUS_LEFT, _ffi.STATUS_FAILED


def state_of(bits):
    """0 for not known, else the status (1 Alive .. 4 Failed)."""
    bits = np.asarray(bits).astype(np.int64)
    return np.where(bits & 1, np.minimum((bits >> 1) & 7, FAILED), 0)


def classify(prev, cur, t, flap_window):
    """The seven counted columns of the transitions prev -> cur (arrays of bits words) sampled behind tick t: bool [7][...],
    and (s(prev), s(cur), both known, swim(prev), swim(cur), Failed -> Alive, its dead time)."""
    prev, cur = np.asarray(prev).astype(np.int64), np.asarray(cur).astype(np.int64)
    sp, sc = state_of(prev), state_of(cur)
    gone = (sp == LEFT) | (sp == FAILED)
    join = ((sp == 0) & (sc != 0)) | (gone & (sc == ALIVE))
    leave = (sc == LEFT) & (sp != 0) & (sp != LEFT)
    failed = (sc == FAILED) & (sp != 0) & (sp != FAILED)
    reap = (sp != 0) & (sc == 0)
    back = (sp == FAILED) & (sc == ALIVE)
    age = (t - (prev >> 11)) & STAMP_MASK
    flap = back & (age < flap_window)
    both = ((prev & cur) & 1) != 0
    wp, wc = (prev >> 4) & 3, (cur >> 4) & 3
    susp = both & (wp == _ffi.SWIM_ALIVE) & (wc == _ffi.SWIM_SUSPECT)
    clr = both & (wp == _ffi.SWIM_SUSPECT) & (wc == _ffi.SWIM_ALIVE)
    return np.array([join, leave, failed, reap, flap, susp, clr]), (sp, sc, both, wp, wc, back, age)


def state(sim):
    """(bits [slot][node], slot_of [subject], running [node]) of the state `sim` is in now."""
    rows = sim.dump(_ffi.ARR_ROWS)
    n = len(rows)
    up = (rows["flags"].astype(np.int64) & RF_UP) != 0
    view = sim.dump(_ffi.ARR_VIEW)
    bits = view["bits"].reshape(view.size // n, n).astype(np.uint32)
    return bits, sim.dump(_ffi.ARR_SLOTMAP).astype(np.int64), up


class GazetteModel:
    """sim_gazette_start / count / read / nodes / subjects / top / stop on a Sim without them.  Create it BEFORE the handle's
    first tick (it follows the baselines from sim_create on); step() advances one tick at a time."""

    def __init__(self, sim, on_tick=None):
        self.sim, self.on_tick = sim, on_tick
        self.n = int(sim.cfg.n_nodes)
        joined = int(sim.cfg.flags) & _ffi.CF_BASELINE_JOINED
        self.base = np.full(self.n, (1 | ALIVE << 1) if joined else 0, np.uint32)
        self.recycles = int(sim.cfg.recycle_interval) != 0          # (without recycling no subject ever loses its slot)
        self.before = state(sim) if self.recycles else None
        self.running = False
        self.samples, self.dropped = [], 0
        self.rehomed = 0                                         # fresh slots whose shadow held ANOTHER subject
        self.ages = []                                           # the dead time of every counted Failed -> Alive join
        self.on_slot = None                                      # test hook: on_slot(t, subject, columns & running [7][n], s(prev) [n])

    # ---- the baselines: what a subject's column is filled with when it gets a slot again ----
    def track(self, due):
        """Behind a tick: the baselines moved on; returns the state when a sample is due (or when recycling needs it anyway)."""
        if not self.recycles:
            return state(self.sim) if due else None
        bits0, slot0, up0 = self.before
        now = state(self.sim)
        lost = np.nonzero((slot0 != NOSLOT) & (now[1] != slot0))[0]
        for x in lost.tolist():
            held = bits0[slot0[x]][up0]
            if len(held):                                        # (the running nodes agree, or the slot would not have gone)
                vals, cnt = np.unique(held, return_counts=True)
                self.base[x] = vals[cnt.argmax()]
        self.before = now
        return now

    # ---- the extension ----
    def start(self, first_tick=0, period=1, capacity=1 << 12, flap_window=60):
        assert not self.running and period > 0 and 0 < capacity <= _ffi.GAZETTE_MAX_SAMPLES and flap_window < (1 << 21)
        self.first, self.period, self.capacity, self.window = max(first_tick, self.sim.tick), period, capacity, flap_window
        self.samples, self.dropped, self.running = [], 0, True
        self.nodes = np.zeros((self.n, COLS), np.uint32)
        self.subj = np.zeros((self.n, COLS), np.uint32)
        self.retake(self.before if self.recycles else state(self.sim))
        self.expect = self.first + 1

    def stop(self):
        assert self.running
        self.running = False
        self.samples, self.dropped = [], 0

    def retake(self, st):
        """The whole shadow := the heads' bits; returns the allocated slots."""
        bits, _, _ = st
        slots, subj = subjects(self.sim)
        self.shadow = {int(a): bits[a].copy() for a in slots.tolist()}
        self.shadow_subject = {int(a): int(x) for a, x in zip(slots.tolist(), subj.tolist())}
        return len(slots)

    def sample(self, st, t):
        """The sample behind tick t of the state st; moves the shadow and the maps."""
        bits, _, up = st
        w = np.zeros(WORDS, np.uint64)
        w[0], w[1] = t + 1, int(up.sum())
        if t + 1 != self.expect:                                 # the first sample behind a restore: the shadow is re-taken
            w[2] = w[3] = self.retake(st)
            return w
        slots, subj = subjects(self.sim)
        w[2] = len(slots)
        node_ev = np.zeros((7, self.n), np.int64)
        mat, swim, hist = np.zeros((5, 5), np.int64), np.zeros((4, 4), np.int64), np.zeros(5, np.int64)
        shadow, shadow_subject = {}, {}
        n_subjects, best = 0, (0, 0)
        for a, x in zip(slots.tolist(), subj.tolist()):
            cur = bits[a]
            if self.shadow_subject.get(a) == x:
                prev = self.shadow[a]
            else:                                                # fresh: the column was filled with the subject's baseline
                prev = np.full(self.n, self.base[x], np.uint32)
                w[3] += 1
                self.rehomed += a in self.shadow_subject
            shadow[a], shadow_subject[a] = cur.copy(), x
            cols, (sp, sc, both, wp, wc, back, age) = classify(prev, cur, t, self.window)
            cols = cols & up[None, :]                            # a stopped process emits nothing
            if self.on_slot:
                self.on_slot(t, x, cols, sp)
            node_ev += cols
            s = cols.sum(axis=1)
            self.subj[x, :7] += s.astype(np.uint32)
            self.subj[x, 7] = max(int(self.subj[x, 7]), int(s[2]))
            n_subjects += int(s[:4].sum() > 0)
            if int(s[2]) > best[0]:                              # (slots ascend, subjects need not: the lowest id on a tie)
                best = (int(s[2]), x)
            elif int(s[2]) == best[0] and best[0] and x < best[1]:
                best = (best[0], x)
            ch = up & (sp != sc)
            np.add.at(mat, (sp[ch], sc[ch]), 1)
            chw = up & both & (wp != wc)
            np.add.at(swim, (wp[chw], wc[chw]), 1)
            bk = up & back
            self.ages += age[bk].tolist()
            np.add.at(hist, np.searchsorted([2, 8, 32, 128], age[bk], side="right"), 1)
        self.shadow, self.shadow_subject = shadow, shadow_subject          # (a slot that is free now: cleared)
        self.nodes[:, :7] += node_ev.T.astype(np.uint32)
        ev = node_ev[:4].sum(axis=0)
        self.nodes[:, 7] = np.maximum(self.nodes[:, 7], ev.astype(np.uint32))
        w[4:29], w[29:45], w[45:52] = mat.reshape(-1), swim.reshape(-1), node_ev.sum(axis=1)
        w[52] = int((ev > 0).sum())
        if ev.max(initial=0) > 0:
            w[53], w[54] = int(ev.max()), int(ev.argmax())       # (argmax: the lowest id)
        w[55] = n_subjects
        if best[0]:
            w[56], w[57] = best[1], best[0]
        w[58:63] = hist
        return w

    def due(self, t):
        return self.running and t >= self.first and (t - self.first) % self.period == 0

    def after_tick(self, t, st):
        if self.due(t):
            if len(self.samples) < self.capacity:
                self.samples.append(self.sample(st, t))
                self.expect = t + 1 + self.period
            else:
                self.dropped += 1                                # (not looked at either: shadow and maps stand)

    def step(self, k=1):
        for _ in range(k):
            t = self.sim.tick
            self.sim.step(1)
            self.after_tick(t, self.track(self.due(t) and len(self.samples) < self.capacity))
            if self.on_tick:
                self.on_tick()

    def restored(self):
        """The handle was restored from an image: the dumps before the next tick are the image's."""
        self.before = state(self.sim) if self.recycles else None

    def count(self):
        return len(self.samples), self.dropped

    def read(self, first=0, n=None):
        sel = self.samples[first:] if n is None else self.samples[first:first + n]
        return np.array(sel, np.uint64).reshape(-1, WORDS).reshape(-1).view(_ffi.GAZETTE_SAMPLE_DTYPE)

    def map(self, which):
        return self.subj if which == _ffi.GAZETTE_MAP_SUBJECTS else self.nodes

    def top(self, which, column, k):
        """ALL rows ranked by a column descending, ties in ascending id: the first k as GAZETTE_RANK_DTYPE."""
        m = self.map(which)
        order = np.lexsort((np.arange(self.n), -m[:, column].astype(np.int64)))[:k]
        out = np.zeros(k, _ffi.GAZETTE_RANK_DTYPE)
        out["id"] = 0xFFFFFFFF
        out["id"][:len(order)] = order
        out["row"][:len(order)] = m[order]
        return out
