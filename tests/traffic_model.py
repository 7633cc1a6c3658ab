"""Reference model of the traffic meter (include/serf_sim_traffic.h): the packets in flight behind a tick taken from the canonical
dumps of any _ffi.Sim — ARR_INBOX for the packets, ARR_ROWS for who runs — and addressed with the tick's target draw:
tests/third_model.py::k_random_nodes under SIM_CF_RANDOM_FANOUT (the inbox is indexed by SENDER: cell [slot][sender]; drawn for
every node at once by k_random_nodes_all, the same draws in numpy), the oracle's osim_t_targets under the bijection (the inbox is
indexed by RECEIVER: cell [slot][target], its sender is the node whose k-th target that is).  From the packets the map, the samples and the three reads of the map, on a handle that is stepped one tick at
a time.  The CPU oracle has no meter; with this model it is the checker of the HIP library's.  The twin of tests/spread_model.py.

tests/test_traffic.py checks the model against routes that do not share its code: the series' and the ledger's totals, the
conservation of packets between senders and targets, the spread map's arrivals."""
import ctypes as C

import numpy as np

from serf_amd import _ffi

WORDS, COLS = _ffi.TRAFFIC_WORDS, _ffi.TRAFFIC_COLUMNS
DEG_BINS, REC_BINS, BINS = _ffi.TRAFFIC_DEG_BINS, _ffi.TRAFFIC_REC_BINS, _ffi.TRAFFIC_BINS
RF_UP = 1
TX_P, TX_R, TX_U, RX_P, RX_R, RX_U, RX_PEAK, RX_DOWN = range(8)


def _mix64(z):
    """splitmix64's finaliser on uint64 arrays (tests/third_model.py::mix64; uint64 arithmetic wraps)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def k_random_nodes_all(seed, tick, n, fanout):
    """k_random_nodes(seed, tick, node, n, fanout) for every node at once: [n][fanout] targets, -1 where a node found fewer.
    The same draws in the same order, in numpy (tests/test_traffic.py compares the two node by node)."""
    with np.errstate(over="ignore"):
        base = _mix64(_mix64(np.array([seed ^ ((7 * 0xD6E8FEB86659FD93) & ((1 << 64) - 1))], np.uint64)) ^ np.uint64(tick))[0]
        node = np.arange(n, dtype=np.uint64)
        chosen = np.full((n, fanout), -1, np.int64)
        found = np.zeros(n, np.int64)
        for i in range(3 * n):
            todo = found < fanout
            if not todo.any():
                break
            t = (((_mix64(base ^ (node * np.uint64(4096) + np.uint64(i))) >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
            ok = todo & (t != np.arange(n)) & ~(chosen == t[:, None]).any(axis=1)
            chosen[ok, found[ok]] = t[ok]
            found += ok
    return chosen


def bijection_targets(sim, tick):
    """osim_t_targets for every node: ([n][feff] targets, feff)."""
    n = int(sim.cfg.n_nodes)
    fn = sim.lib.t["targets"]
    out = (C.c_uint32 * 4)()
    rows, feff = [], 0
    for g in range(n):
        feff = fn(sim.h, tick, g, out)
        assert feff >= 0
        rows.append(list(out[:feff]))
    return np.array(rows, np.int64).reshape(n, feff), feff


def packets(sim):
    """The packets in flight of the state `sim` is in now (sent during tick sim.tick - 1), flat: (sender, target, records, units)
    arrays, one element per (sender, slot) with at least one non-empty record; and the running mask."""
    n, fanout = int(sim.cfg.n_nodes), int(sim.cfg.fanout)
    up = (sim.dump(_ffi.ARR_ROWS)["flags"].astype(np.int64) & RF_UP) != 0
    empty = np.zeros(0, np.int64)
    if sim.tick == 0:
        return empty, empty, empty, empty, up
    hm = sim.dump(_ffi.ARR_INBOX).reshape(-1, n)["hi_meta"].astype(np.int64)       # [fanout * pg][node][4]
    pg = hm.shape[0] // fanout
    full = (((hm >> 4) & 0xF) != 0).reshape(fanout, pg, n, 4)
    length = (63 - ((hm >> 8) & 0x3F)).reshape(fanout, pg, n, 4)
    rec = full.sum(axis=(1, 3))                                                      # [fanout][node]
    units = np.where(full, length, 0).sum(axis=(1, 3))
    slot, cell = np.nonzero(rec > 0)
    t = sim.tick - 1
    if int(sim.cfg.flags) & _ffi.CF_RANDOM_FANOUT:
        tg = k_random_nodes_all(int(sim.cfg.seed), t, n, fanout)
        sender, target = cell, tg[cell, slot]
        assert (target >= 0).all(), "a packet in a slot that drew no target"
    else:
        tg, feff = bijection_targets(sim, t)
        assert (slot < feff).all(), "a packet in a slot beyond the tick's fan-out"
        src = np.full((fanout, n), -1, np.int64)
        for k in range(feff):
            src[k, tg[:, k]] = np.arange(n)
        sender, target = src[slot, cell], cell
        assert (sender >= 0).all()
    return sender, target, rec[slot, cell], units[slot, cell], up


def ranked(nodes, up, column, top_k):
    """sim_traffic_top from every node's record: TRAFFIC_RANK_DTYPE [top_k]."""
    n = len(nodes)
    val = nodes[_ffi.TRAFFIC_COLUMN_NAMES[column]].astype(np.int64)
    order = np.lexsort((np.arange(n), -val))[:top_k]
    top = np.zeros(top_k, _ffi.TRAFFIC_RANK_DTYPE)
    top["id"] = 0xFFFFFFFF
    top["id"][:len(order)] = order
    top["running"][:len(order)] = up[order]
    top["node"][:len(order)] = nodes[order]
    return top


class TrafficModel:
    """sim_traffic_start / count / read / stop / nodes / top / summary on a Sim without them: step() advances one tick at a time
    and accumulates behind the ticks the rule of include/serf_sim_traffic.h names."""

    def __init__(self, sim, on_tick=None):
        self.sim, self.on_tick = sim, on_tick
        self.running = False
        self.samples, self.dropped = [], 0

    def start(self, first_tick=0, period=1, capacity=1 << 12):
        assert not self.running and period > 0 and 0 < capacity <= _ffi.TRAFFIC_MAX_SAMPLES
        self.first, self.period, self.capacity = max(first_tick, self.sim.tick), period, capacity
        self.map = np.zeros((COLS, int(self.sim.cfg.n_nodes)), np.uint32)
        self.samples, self.dropped, self.running = [], 0, True

    def stop(self):
        assert self.running
        self.running = False
        self.samples, self.dropped = [], 0

    def sample(self):
        """Adds the packets in flight now (after tick sim.tick - 1) to the map and returns the sample's 64 words."""
        n = int(self.sim.cfg.n_nodes)
        sender, target, rec, units, up = packets(self.sim)

        def per(idx, weight=None):
            return np.bincount(idx, weights=weight, minlength=n).astype(np.int64)
        deg, rx_units = per(target), per(target, units)
        add = np.zeros((COLS, n), np.int64)
        add[TX_P], add[TX_R], add[TX_U] = per(sender), per(sender, rec), per(sender, units)
        add[RX_P], add[RX_R], add[RX_U] = deg, per(target, rec), rx_units
        add[RX_DOWN] = np.where(up, 0, deg)
        self.map += add.astype(np.uint32)                                              # (uint32: wraps as the device's additions do)
        self.map[RX_PEAK] = np.maximum(self.map[RX_PEAK], deg.astype(np.uint32))
        w = np.zeros(WORDS, np.uint64)
        w[0], w[1], w[2], w[3], w[4] = self.sim.tick, int(up.sum()), len(rec), int(rec.sum()), int(units.sum())
        w[5], w[6], w[7] = int((add[TX_P] > 0).sum()), int((deg > 0).sum()), int(deg[~up].sum())
        if deg.max(initial=0) > 0:
            w[8], w[9] = int(deg.max()), int(np.argmax(deg))                           # (argmax: the first = the smallest id)
        if rx_units.max(initial=0) > 0:
            w[10], w[11] = int(rx_units.max()), int(np.argmax(rx_units))
        w[12], w[13] = int(rec.max(initial=0)), int(units.max(initial=0))
        w[14] = len(self.samples) + 1
        w[16:16 + DEG_BINS] = np.bincount(np.minimum(deg, DEG_BINS - 1), minlength=DEG_BINS)
        w[48:48 + REC_BINS] = np.bincount(rec, minlength=REC_BINS + 1)[1:REC_BINS + 1]
        return w

    def after_tick(self, t):
        """Tick t has just run (by whoever steps the handle): its sample, when one is due."""
        if self.running and t >= self.first and (t - self.first) % self.period == 0:
            if len(self.samples) < self.capacity:
                self.samples.append(self.sample())
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
        """Samples first .. first + n - 1 as Sim.traffic_read returns them (TRAFFIC_DTYPE)."""
        sel = self.samples[first:] if n is None else self.samples[first:first + n]
        return np.ascontiguousarray(np.array(sel, np.uint64).reshape(-1, WORDS)).view(_ffi.TRAFFIC_DTYPE).reshape(-1)

    # ---- the reads of the map: from the map and the running flags the handle has now ----
    def nodes(self, first_node=0, count=None):
        sel = self.map[:, first_node:None if count is None else first_node + count]
        return np.ascontiguousarray(sel.T).view(_ffi.TRAFFIC_NODE_DTYPE).reshape(-1)

    def top(self, top_k=10, column=5):
        up = (self.sim.dump(_ffi.ARR_ROWS)["flags"].astype(np.int64) & RF_UP) != 0
        return ranked(self.nodes(), up, column, top_k)

    def summary(self, column=5, bin_width=1):
        assert 0 <= column < COLS and bin_width > 0
        v = self.map[column].astype(np.int64)
        out = np.zeros(1, _ffi.TRAFFIC_SUMMARY_DTYPE)[0]
        out["column"], out["bin_width"], out["sum"], out["max"], out["max_id"] = column, bin_width, v.sum(), v.max(), np.argmax(v)
        out["min"], out["nonzero"], out["samples"] = v.min(), (v != 0).sum(), len(self.samples)
        out["bins"] = np.bincount(np.minimum(v // bin_width, BINS - 1), minlength=BINS)
        return out
