"""Reference model of the device-resident time series (include/serf_sim_series.h): the 64 words of a sample computed with
numpy from the canonical dumps (ARR_ROWS / ARR_QUEUE / ARR_INBOX) of any _ffi.Sim, and the sampling rule on a handle that is
stepped one tick at a time.  The CPU oracle has no series; with this model it is the checker of the HIP library's."""
import numpy as np

from serf_amd import _ffi

WORDS = 64
META_EMPTY = 0xFFFFFFFF
RF_UP = 1


def sample(sim, running_only=True):
    """The sample of the state `sim` is in now (after tick sim.tick - 1), as 64 unsigned 64-bit words.  running_only=False
    sums the per-node figures over ALL nodes (what sim_cluster_stats does): for the cross-check against that route only."""
    rows = sim.dump(_ffi.ARR_ROWS)
    n = len(rows)
    queue = sim.dump(_ffi.ARR_QUEUE).reshape(n, -1)
    inbox = sim.dump(_ffi.ARR_INBOX).reshape(-1, n)           # [fanout * PG][node] pages
    w = np.zeros(WORDS, np.uint64)
    flags = rows["flags"].astype(np.int64)
    up = (flags & RF_UP) != 0
    sel = up if running_only else np.ones(n, bool)
    r = rows[sel]
    w[0] = sim.tick
    w[1] = int(up.sum())                              # (running nodes, whatever the switch says)
    state = (flags[sel] >> 1) & 3
    for i in range(4):
        w[2 + i] = int((state == i).sum())
    meta = queue["meta"][sel]
    full = meta != META_EMPTY
    cls = meta >> 30
    for c in range(4):
        w[6 + c] = int((full & (cls == c)).sum())
    depth = full.sum(axis=1).astype(np.int64)
    bins = np.where(depth == 0, 0, 1 + np.floor(np.log2(np.maximum(depth, 1))).astype(np.int64))
    for b in range(8):
        w[10 + b] = int((bins == b).sum())
    assert int(w[10:18].sum()) == int(sel.sum())      # (a depth is at most 64: eight bins hold every node)
    w[18] = int(depth.max()) if len(depth) else 0
    for a in range(8):
        w[19 + a] = int((r["awareness"] == a).sum())
    timers = (r["susp"] != 0).sum(axis=1)
    w[27] = int(timers.sum())
    w[28] = int((timers > 0).sum())
    w[29] = int(r["n_failed"].astype(np.int64).sum())
    w[30] = int(r["n_left"].astype(np.int64).sum())
    if len(r):
        w[31], w[32] = int(r["n_known"].min()), int(r["n_known"].max())
        for i, f in enumerate(("clock", "event_clock", "query_clock")):
            w[33 + 2 * i], w[34 + 2 * i] = int(r[f].min()), int(r[f].max())
    w[39] = int(rows["overflow"].astype(np.int64).sum())          # ALL nodes, always: the model-bound counter
    hm = inbox["hi_meta"].astype(np.int64)                        # [pages][node][4]
    kind = (hm >> 4) & 0xF
    fanout = int(sim.cfg.fanout)
    pg = hm.shape[0] // fanout
    has = (kind != 0).reshape(fanout, pg, n, 4).any(axis=(1, 3))  # a packet = the pg pages of one (slot, node)
    w[40] = int(has.sum())
    for k in range(1, 8):
        w[40 + k] = int((kind == k).sum())
    w[48] = int((63 - ((hm >> 8) & 0x3F))[kind != 0].sum())
    return w


def as_records(words):
    """[samples][64] words -> a numpy array of _ffi.SERIES_DTYPE (the field names of the table)."""
    a = np.ascontiguousarray(np.asarray(words, np.uint64).reshape(-1, WORDS))
    return a.view(_ffi.SERIES_DTYPE).reshape(-1)


class SeriesModel:
    """sim_series_start / count / read / stop on a Sim without them: step() advances one tick at a time and takes the
    samples the rule of include/serf_sim_series.h asks for."""

    def __init__(self, sim, on_tick=None):
        self.sim, self.on_tick = sim, on_tick
        self.running = False
        self.samples, self.dropped = [], 0

    def start(self, first_tick=0, period=1, capacity=1 << 16):
        assert not self.running and period > 0 and 0 < capacity <= _ffi.SERIES_MAX_SAMPLES
        self.first, self.period, self.capacity = max(first_tick, self.sim.tick), period, capacity
        self.samples, self.dropped, self.running = [], 0, True

    def stop(self):
        assert self.running
        self.running = False
        self.samples, self.dropped = [], 0

    def step(self, k=1):
        for _ in range(k):
            t = self.sim.tick
            self.sim.step(1)
            if self.running and t >= self.first and (t - self.first) % self.period == 0:
                if len(self.samples) < self.capacity:
                    self.samples.append(sample(self.sim))
                else:
                    self.dropped += 1
            if self.on_tick:
                self.on_tick()

    def count(self):
        return len(self.samples), self.dropped

    def read(self):
        return np.array(self.samples, np.uint64).reshape(-1, WORDS)
