"""Reference model of the membership census (include/serf_sim_census.h): a sample — the header and the subjects' records —
computed with numpy from the canonical dumps (ARR_VIEW / ARR_SLOTMAP / ARR_ROWS) of any _ffi.Sim, and the sampling rule on a
handle that is stepped one tick at a time.  The CPU oracle has no census; with this model it is the checker of the HIP
library's."""
import numpy as np

from serf_amd import _ffi

WORDS = _ffi.CENSUS_WORDS
NOSLOT = 0xFFFFFFFF
RF_UP = 1


def subjects(sim):
    """(slots ascending, their subjects): ARR_SLOTMAP is slot_of[subject]; inverted here."""
    slot_of = sim.dump(_ffi.ARR_SLOTMAP).astype(np.int64)
    subj = np.nonzero(slot_of != NOSLOT)[0]
    order = np.argsort(slot_of[subj], kind="stable")
    return slot_of[subj][order], subj[order]


def sample(sim, max_subjects):
    """The sample of the state `sim` is in now (after tick sim.tick - 1): (1 + max_subjects) * 16 unsigned 64-bit words."""
    rows = sim.dump(_ffi.ARR_ROWS)
    n = len(rows)
    up = (rows["flags"].astype(np.int64) & RF_UP) != 0
    view = sim.dump(_ffi.ARR_VIEW)
    view = view.reshape(view.size // n, n)                      # [slot][observer]
    slots, subj = subjects(sim)
    running, ns = int(up.sum()), len(slots)
    e = view[slots][:, up]                                      # [subject][running observer]
    bits = e["bits"].astype(np.int64)
    known = (bits & 1) != 0
    st = np.where(known, (bits >> 1) & 7, _ffi.STATUS_NONE)
    swim = (bits >> 4) & 3
    w = np.zeros((ns, WORDS), np.uint64)
    w[:, 0] = subj | (slots << 32)
    w[:, 1] = up[subj]
    for b in range(5):
        w[:, 2 + b] = (st == b).sum(axis=1)
    for b in range(4):
        w[:, 7 + b] = (known & (swim == b)).sum(axis=1)
    w[:, 11] = (~known & (((bits >> 6) & 3) != 0)).sum(axis=1)
    anyk = known.any(axis=1)
    big = np.uint64(0xFFFFFFFFFFFFFFFF)
    lt, inc = e["ltime"].astype(np.uint64), e["inc"].astype(np.uint64)
    if running:
        w[:, 12] = np.where(anyk, np.where(known, lt, big).min(axis=1), 0)
        w[:, 13] = np.where(known, lt, 0).max(axis=1)
        w[:, 14] = np.where(anyk, np.where(known, inc, big).min(axis=1), 0)
        w[:, 15] = np.where(known, inc, 0).max(axis=1)
    c, s = w[:, 2:7].astype(np.int64), w[:, 7:11].astype(np.int64)
    assert (c.sum(axis=1) == running).all() and (s.sum(axis=1) == running - c[:, 0]).all()
    hdr = np.zeros(WORDS, np.uint64)
    hdr[0], hdr[1], hdr[2], hdr[3] = sim.tick, running, ns, min(ns, max_subjects)
    if running and ns:
        settled = (c[:, 0] == running) | ((c[:, 1:] == running).any(axis=1) & (s == running).any(axis=1)
                                          & (w[:, 12] == w[:, 13]) & (w[:, 14] == w[:, 15]))
        run = up[subj]
        failed, bad, alive = c[:, _ffi.STATUS_FAILED], s[:, _ffi.SWIM_SUSPECT] + s[:, _ffi.SWIM_DEAD], c[:, _ffi.STATUS_ALIVE]
        hdr[4] = int(settled.sum())
        hdr[5], hdr[6] = int((run & (failed > 0)).sum()), int(failed[run].sum())
        hdr[7], hdr[8] = int((run & (bad > 0)).sum()), int(bad[run].sum())
        hdr[9], hdr[10] = int((~run & (alive > 0)).sum()), int(alive[~run].sum())
        hdr[11] = int((~run & (failed + c[:, _ffi.STATUS_LEFT] == running)).sum())
    out = np.zeros((1 + max_subjects, WORDS), np.uint64)
    out[0] = hdr
    k = min(ns, max_subjects)
    out[1:1 + k] = w[:k]
    return out.reshape(-1)


def split(words, max_subjects):
    """Words of whole samples -> (headers[samples], records[samples][max_subjects]) with the fields' names."""
    return _ffi.census_split(words, max_subjects)


class CensusModel:
    """sim_census_start / count / read / stop / now on a Sim without them: step() advances one tick at a time and takes the
    samples the rule of include/serf_sim_census.h asks for."""

    def __init__(self, sim, on_tick=None):
        self.sim, self.on_tick = sim, on_tick
        self.running = False
        self.samples, self.dropped = [], 0

    def start(self, first_tick=0, period=1, capacity=1 << 12, max_subjects=64):
        assert not self.running and period > 0 and 0 < capacity <= _ffi.CENSUS_MAX_SAMPLES and max_subjects > 0
        self.first, self.period, self.capacity = max(first_tick, self.sim.tick), period, capacity
        self.max_subjects = max_subjects
        self.samples, self.dropped, self.running = [], 0, True

    def stop(self):
        assert self.running
        self.running = False
        self.samples, self.dropped = [], 0

    def after_tick(self, t):
        """Tick t has just run (by whoever steps the handle): its sample, when one is due."""
        if self.running and t >= self.first and (t - self.first) % self.period == 0:
            if len(self.samples) < self.capacity:
                self.samples.append(sample(self.sim, self.max_subjects))
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
        return len(self.samples), self.dropped

    def read(self, first=0, n=None):
        """(headers, records) of samples first .. first + n - 1, as Sim.census_read returns them."""
        sel = self.samples[first:] if n is None else self.samples[first:first + n]
        return split(np.array(sel, np.uint64).reshape(-1), self.max_subjects)

    def now(self, cap=64):
        """(header, records[min(subjects, cap)]) of the state the handle is in, as Sim.census_now returns it."""
        hdr, rec = split(sample(self.sim, max(cap, 1)), max(cap, 1))
        h = hdr[0].copy()
        h["stored"] = min(int(h["subjects"]), cap)
        return h, rec[0][:int(h["stored"])]
