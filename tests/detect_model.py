"""Reference model of the detection log (include/serf_sim_detect.h): a pure-Python fold of the header's rules over the census
records (tests/census_model.sample) of the sampled ticks of any _ffi.Sim, with the sampling rule of CensusModel.  The CPU
oracle has no detection log; with this model it is the checker of the HIP library's."""
import numpy as np

from serf_amd import _ffi
from tests import census_model

NEVER = _ffi.DETECT_NEVER
DOWN, ACCUSED = _ffi.DETECT_DOWN, _ffi.DETECT_ACCUSED
DETECTED, RETURNED, CLEARED, STOPPED, ABANDONED = 1, 2, 3, 4, 5
CENSORED, AFTER_RETURN = _ffi.DETECT_F_CENSORED, _ffi.DETECT_F_AFTER_RETURN
CW = _ffi.CENSUS_WORDS


def view_slots_of(sim):
    c = sim.cfg
    return c.n_nodes if c.view_slots == 0 or c.view_slots >= c.n_nodes else c.view_slots


def census_inputs(sim):
    """What one evaluation reads: (now, R, {slot: (subject, run, failed, left, susp)}) of the state `sim` is in."""
    a = view_slots_of(sim)
    w = census_model.sample(sim, a).reshape(1 + a, CW)
    hdr, rec = w[0], w[1:1 + int(w[0][2])]
    slots = {}
    for r in rec:
        r = [int(x) for x in r]
        slots[r[0] >> 32] = (r[0] & 0xFFFFFFFF, r[1] & 1, r[6], r[5], r[8] + r[9])
    return int(hdr[0]), int(hdr[1]), slots


def new_episode(kind, subject, slot, now, flags):
    return dict(subject=subject, slot=slot, kind=kind, outcome=0, flags=flags, opened=now, closed=NEVER,
                first_suspect=now if kind == ACCUSED else NEVER, first_failed=NEVER, half=NEVER, p99=NEVER, all=NEVER,
                evaluated=0, peak=0, peak_susp=0)


def as_records(episodes):
    out = np.zeros(len(episodes), _ffi.DETECT_EPISODE_DTYPE)
    for i, e in enumerate(episodes):
        for k, v in e.items():
            out[k][i] = v
    return out


class DetectFold:
    """The state machine alone: evaluate(now, R, slots) once per sample."""

    def __init__(self, log_capacity):
        self.log_capacity = log_capacity
        self.state = {}          # slot -> dict(subject, prev_run, done, ep)
        self.log, self.lost = [], 0
        self.cum = np.zeros(_ffi.DETECT_WORDS, np.uint64)   # words 8 .. 63: the cumulative ones
        self.samples = 0

    def _close(self, ep, outcome, now, closed):
        ep = dict(ep, outcome=outcome, closed=now)
        closed.append(ep)
        c = self.cum
        c[8 + outcome - 1] += 1
        if ep["kind"] == ACCUSED and ep["first_failed"] != NEVER:
            c[13] += 1
        if outcome == DETECTED and not ep["flags"] & CENSORED:
            fs = ep["first_suspect"]
            c[16 + (15 if fs == NEVER else _ffi.detect_bin(fs - ep["opened"]))] += 1
            c[32 + _ffi.detect_bin(ep["all"] - ep["opened"])] += 1
        if outcome == CLEARED:
            c[48 + _ffi.detect_bin(now - ep["opened"])] += 1

    def _open(self, kind, subject, slot, now, flags):
        self.cum[14 if kind == DOWN else 15] += 1
        return new_episode(kind, subject, slot, now, flags)

    def evaluate(self, now, R, slots):
        """slots: {slot: (subject, run, failed, left, susp)} of the slots that have a subject.  Returns the header's words."""
        first_sample = self.samples == 0
        closed = []
        for a in sorted(set(self.state) | set(slots)):
            s, cur = self.state.get(a), slots.get(a)
            fresh = False
            if s is None or cur is None or s["subject"] != cur[0]:            # 1. subject change
                if s is not None and s["ep"] is not None:
                    self._close(s["ep"], ABANDONED, now, closed)
                self.state.pop(a, None)
                if cur is None:
                    continue
                fresh = True
                s = self.state[a] = dict(subject=cur[0], prev_run=0, done=False, ep=None)
            subject, run, failed, left, susp = cur
            gone = failed + left
            ep = s["ep"]
            if run:                                                           # 2. the subject runs
                returned = False
                if ep is not None and ep["kind"] == DOWN:
                    self._close(ep, RETURNED, now, closed)
                    ep, returned = None, True
                s["done"] = False
                if susp > 0 or failed > 0:
                    if ep is None:
                        ep = self._open(ACCUSED, subject, a, now, AFTER_RETURN if returned else 0)
                    if failed > 0 and ep["first_failed"] == NEVER:
                        ep["first_failed"] = now
                    ep["peak"], ep["peak_susp"] = max(ep["peak"], failed), max(ep["peak_susp"], susp)
                    ep["evaluated"] += 1
                elif ep is not None:
                    self._close(ep, CLEARED, now, closed)
                    ep = None
            else:                                                             # 3. the subject is stopped
                if (ep is None or ep["kind"] != DOWN) and not s["done"] and (fresh or s["prev_run"]):
                    if ep is not None:
                        self._close(ep, STOPPED, now, closed)
                    ep = self._open(DOWN, subject, a, now, CENSORED if fresh and first_sample else 0)
                if ep is not None and ep["kind"] == DOWN:
                    for name, ok in (("first_suspect", susp > 0 or failed > 0), ("first_failed", failed > 0),
                                     ("half", R > 0 and 2 * gone >= R), ("p99", R > 0 and 100 * gone >= 99 * R),
                                     ("all", R > 0 and gone == R)):
                        if ok and ep[name] == NEVER:
                            ep[name] = now
                    ep["peak"], ep["peak_susp"] = max(ep["peak"], gone), max(ep["peak_susp"], susp)
                    ep["evaluated"] += 1
                    if ep["all"] != NEVER:
                        self._close(ep, DETECTED, now, closed)
                        ep, s["done"] = None, True
            s["ep"] = ep
            s["prev_run"] = run                                               # 4.
        for ep in closed:
            if len(self.log) < self.log_capacity:
                self.log.append(ep)
            else:
                self.lost += 1
        self.samples += 1
        h = self.cum.copy()
        opened = self.open()
        h[0], h[1], h[2] = now, R, len(slots)
        h[3], h[4] = sum(e["kind"] == DOWN for e in opened), sum(e["kind"] == ACCUSED for e in opened)
        h[5], h[6], h[7] = len(closed), len(self.log), self.lost
        return h

    def open(self):
        return [dict(s["ep"]) for a, s in sorted(self.state.items()) if s["ep"] is not None]


class DetectModel:
    """sim_detect_start / count / read / log / open / stop on a Sim without them: step() advances one tick at a time and
    evaluates behind the ticks the rule of include/serf_sim_detect.h samples."""

    def __init__(self, sim, on_tick=None):
        self.sim, self.on_tick = sim, on_tick
        self.running = False
        self.headers, self.dropped, self.fold = [], 0, None

    def start(self, first_tick=0, period=1, capacity=1 << 12, log_capacity=1 << 16):
        assert not self.running and period > 0 and 0 < capacity <= _ffi.DETECT_MAX_SAMPLES and 0 < log_capacity <= _ffi.DETECT_MAX_LOG
        self.first, self.period, self.capacity = max(first_tick, self.sim.tick), period, capacity
        self.headers, self.dropped, self.running = [], 0, True
        self.fold = DetectFold(log_capacity)

    def stop(self):
        assert self.running
        self.running = False
        self.headers, self.dropped, self.fold = [], 0, None

    def after_tick(self, t):
        """Tick t has just run (by whoever steps the handle): its evaluation, when one is due."""
        if self.running and t >= self.first and (t - self.first) % self.period == 0:
            if len(self.headers) < self.capacity:
                self.headers.append(self.fold.evaluate(*census_inputs(self.sim)))
            else:
                self.dropped += 1

    def step(self, k=1):
        for _ in range(k):
            t = self.sim.tick
            self.sim.step(1)
            self.after_tick(t)
            if self.on_tick:
                self.on_tick()

    def count(self):
        return len(self.headers), self.dropped

    def read(self, first=0, n=None):
        """The headers of samples first .. first + n - 1, as Sim.detect_read returns them."""
        sel = self.headers[first:] if n is None else self.headers[first:first + n]
        return np.array(sel, np.uint64).reshape(-1, _ffi.DETECT_WORDS).view(_ffi.DETECT_HEADER_DTYPE).reshape(-1)

    def log_count(self):
        return len(self.fold.log), self.fold.lost

    def log(self, first=0, n=None):
        """Log records first .. first + n - 1, as Sim.detect_log returns them."""
        return as_records(self.fold.log[first:] if n is None else self.fold.log[first:first + n])

    def open(self):
        """The episodes still open, as Sim.detect_open returns them."""
        return as_records(self.fold.open())
