"""Reference model of the observer roll (include/serf_sim_roll.h): a sample — the header, the listed observers and every node's
record — computed with numpy from the canonical dumps (ARR_VIEW / ARR_SLOTMAP / ARR_ROWS) of any _ffi.Sim, and the sampling
rule on a handle that is stepped one tick at a time.  The CPU oracle has no roll; with this model it is the checker of the
HIP library's.  The twin of tests/census_model.py."""
import numpy as np

from serf_amd import _ffi
from tests.census_model import RF_UP, subjects

HW, NW = _ffi.ROLL_HEADER_WORDS, _ffi.ROLL_NODE_WORDS
BY = (_ffi.ROLL_BY_STALE, _ffi.ROLL_BY_ACCUSED, _ffi.ROLL_BY_MISSED)


def node_records(sim):
    """(records [n_nodes][8] as unsigned 64-bit words, running [n_nodes], number of subjects) of the state `sim` is in now."""
    rows = sim.dump(_ffi.ARR_ROWS)
    n = len(rows)
    up = (rows["flags"].astype(np.int64) & RF_UP) != 0
    view = sim.dump(_ffi.ARR_VIEW)
    view = view.reshape(view.size // n, n)                      # [slot][node]
    slots, subj = subjects(sim)
    e = view[slots]                                             # [subject][node]
    bits = e["bits"].astype(np.int64)
    known = (bits & 1) != 0
    st, swim = (bits >> 1) & 7, (bits >> 4) & 3
    lt, inc = e["ltime"].astype(np.uint64), e["inc"].astype(np.int64)
    seen = known & up[None, :]                                  # known entries of the observers
    # per subject, over the observers whose entry is known
    ltmax = np.where(seen, lt, np.uint64(0)).max(axis=1, initial=np.uint64(0))[:, None]
    incmax = np.where(seen, inc, 0).max(axis=1, initial=0)[:, None]
    anyknown = seen.any(axis=1)[:, None]
    run = up[subj][:, None]
    w = np.zeros((n, NW), np.uint64)
    unknown = (~known & anyknown).sum(axis=0)
    behind = (known & ((lt < ltmax) | (inc < incmax))).sum(axis=0)
    w[:, 0] = np.arange(n, dtype=np.uint64) | (up.astype(np.uint64) << np.uint64(32))
    w[:, 1] = unknown + behind
    w[:, 2] = unknown
    w[:, 3] = (run & known & (st == _ffi.STATUS_FAILED)).sum(axis=0)
    w[:, 4] = (run & known & ((swim == _ffi.SWIM_SUSPECT) | (swim == _ffi.SWIM_DEAD))).sum(axis=0)
    w[:, 5] = (~run & known & (st == _ffi.STATUS_ALIVE)).sum(axis=0)
    w[:, 6] = np.where(seen, ltmax - np.where(seen, lt, ltmax), np.uint64(0)).sum(axis=0, dtype=np.uint64)
    w[:, 7] = behind
    w[~up, 1:] = 0                                              # a node that does not run observes nothing
    return w, up, len(slots)


def score_of(w, rank_by):
    return {_ffi.ROLL_BY_STALE: w[:, 1], _ffi.ROLL_BY_ACCUSED: w[:, 3] + w[:, 4], _ffi.ROLL_BY_MISSED: w[:, 5]}[rank_by].astype(np.int64)


def stale_bin(stale):
    """Bin 0 holds stale == 0; otherwise 1 + floor(log2(stale)), capped at 15."""
    return 0 if stale == 0 else min(int(stale).bit_length(), 15)


def header_and_top(sim_tick, w, up, n_subjects, top_k, rank_by):
    hdr = np.zeros(HW, np.uint64)
    o = w[up].astype(np.int64)                                  # the observers' records ([:, 6] stays below 2^63 in any run)
    score = score_of(w, rank_by)
    order = np.lexsort((np.arange(len(w)), -score))             # descending score, ties in ascending id
    listed = [i for i in order[:top_k].tolist() if score[i] > 0 and up[i]]
    hdr[0], hdr[1], hdr[2], hdr[3] = sim_tick, len(o), n_subjects, len(listed) | (rank_by << 32)
    if len(o):
        hdr[4] = int((o[:, 1] == 0).sum())
        hdr[5], hdr[6], hdr[7] = int(o[:, 1].sum()), int(o[:, 1].max()), int(o[:, 2].sum())
        for j, col in ((8, 3), (10, 4), (12, 5)):
            hdr[j], hdr[j + 1] = int((o[:, col] > 0).sum()), int(o[:, col].sum())
        hdr[14], hdr[15] = int(o[:, 6].sum()), int(o[:, 6].max())
        hdr[16:32] = np.bincount([stale_bin(x) for x in o[:, 1].tolist()], minlength=16)
    top = np.zeros((top_k, NW), np.uint64)
    top[:len(listed)] = w[listed]
    return hdr, top


def sample(sim, top_k, rank_by):
    """The sample of the state `sim` is in now (after tick sim.tick - 1): 32 + 8 * top_k unsigned 64-bit words."""
    assert 1 <= top_k <= _ffi.ROLL_TOP_MAX and rank_by in BY
    w, up, ns = node_records(sim)
    hdr, top = header_and_top(sim.tick, w, up, ns, top_k, rank_by)
    return np.concatenate([hdr, top.reshape(-1)])


def split(words, top_k):
    """Words of whole samples -> (headers[samples], records[samples][top_k]) with the fields' names."""
    return _ffi.roll_split(words, top_k)


class RollModel:
    """sim_roll_start / count / read / stop / now on a Sim without them: step() advances one tick at a time and takes the
    samples the rule of include/serf_sim_roll.h asks for."""

    def __init__(self, sim, on_tick=None):
        self.sim, self.on_tick = sim, on_tick
        self.running = False
        self.samples, self.dropped = [], 0

    def start(self, first_tick=0, period=1, capacity=1 << 12, top_k=8, rank_by=_ffi.ROLL_BY_STALE):
        assert not self.running and period > 0 and 0 < capacity <= _ffi.ROLL_MAX_SAMPLES
        assert 1 <= top_k <= _ffi.ROLL_TOP_MAX and rank_by in BY
        self.first, self.period, self.capacity = max(first_tick, self.sim.tick), period, capacity
        self.top_k, self.rank_by = top_k, rank_by
        self.samples, self.dropped, self.running = [], 0, True

    def stop(self):
        assert self.running
        self.running = False
        self.samples, self.dropped = [], 0

    def after_tick(self, t):
        """Tick t has just run (by whoever steps the handle): its sample, when one is due."""
        if self.running and t >= self.first and (t - self.first) % self.period == 0:
            if len(self.samples) < self.capacity:
                self.samples.append(sample(self.sim, self.top_k, self.rank_by))
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
        """(headers, records) of samples first .. first + n - 1, as Sim.roll_read returns them."""
        sel = self.samples[first:] if n is None else self.samples[first:first + n]
        return split(np.array(sel, np.uint64).reshape(-1), self.top_k)

    def now(self, top_k=8, rank_by=_ffi.ROLL_BY_STALE, nodes=False):
        """(header, top[top_k]) of the state the handle is in — with nodes=True every node's record as well — as
        Sim.roll_now returns them."""
        w, up, ns = node_records(self.sim)
        hdr, top = header_and_top(self.sim.tick, w, up, ns, top_k, rank_by)
        h = hdr.view(_ffi.ROLL_HEADER_DTYPE)[0]
        t = np.ascontiguousarray(top).view(_ffi.ROLL_NODE_DTYPE).reshape(-1)
        return (h, t, np.ascontiguousarray(w).view(_ffi.ROLL_NODE_DTYPE).reshape(-1)) if nodes else (h, t)
