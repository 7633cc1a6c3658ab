"""Reference model of the spread map (include/serf_sim_spread.h): the per-node predicate "has node l applied this rumour?",
computed with numpy from the canonical dumps of any _ffi.Sim — ARR_ROWS / ARR_VIEW / ARR_SLOTMAP for JOIN / LEAVE, with
tests/track_model.py's baseline rules for subjects without a view slot; ARR_ERING / ARR_QRING for EVENT / QUERY, the
overflow rows of ring_overflow > 0 included — the map latched from it on a handle that is stepped one tick at a time, the
samples, and the four reads of the map.  The CPU oracle has no spread map; with this model it is the checker of the HIP
library's.  The twin of tests/ledger_model.py.

The predicate's sum over the running nodes is sim_convergence_many's `seen` (tests/test_spread.py compares them at every
tick: the model cannot drift from the library's predicate unnoticed)."""
import numpy as np

from serf_amd import _ffi
from tests.track_model import TrackModel

HW, EW = _ffi.SPREAD_HEADER_WORDS, _ffi.SPREAD_ENTRY_WORDS
RF_UP = 1
RUMOUR_KINDS = (_ffi.K_JOIN, _ffi.K_LEAVE, _ffi.K_EVENT, _ffi.K_QUERY)


def check_entries(sim, entries):
    n = int(sim.cfg.n_nodes)
    assert 1 <= len(entries) <= _ffi.SPREAD_MAX and len(set(entries)) == len(entries)
    for kind, key, ltime in entries:
        assert kind in RUMOUR_KINDS
        assert (key != 0) if kind in (_ffi.K_EVENT, _ffi.K_QUERY) else key < n
        assert ltime < (1 << 48)


def running(sim):
    return (sim.dump(_ffi.ARR_ROWS)["flags"].astype(np.int64) & RF_UP) != 0


def ring_holds(ring, x, b, key, ltime):
    """bucket_holds (serf_sim_observe.inc) for every node: ring = the dump [x + b][N] of sim_bucket, x overflow rows in front.
    A bucket's keys fill in order — its own six, then its overflow rows in ascending row order — so the tail is looked at only
    behind a full head pair, the overflow rows only behind a full bucket, and a free row ends their walk."""
    idx = int(ltime % b)
    k = ring[x + idx]["keys"].astype(np.int64)                       # [N][6]
    hit = (k[:, 0] == key) | (k[:, 1] == key)
    tail = ~hit & (k[:, 1] != 0)
    hit |= tail & (k[:, 2:] == key).any(axis=1)
    walk = ~hit & tail & (k[:, 5] != 0) & (key != 0)                   # nodes still walking the overflow rows
    for j in range(x):
        row = ring[j]
        owner = row["ltime"].astype(np.int64) & 0xFFFFFFFF
        rk = row["keys"].astype(np.int64)
        walk &= owner != 0                                             # a free row: the walk ends
        mine = walk & (owner == idx + 1)
        head = mine & ((rk[:, 0] == key) | (rk[:, 1] == key))
        hit |= head
        walk &= ~head
        ended = mine & ~head & (rk[:, 1] == 0)
        walk &= ~ended
        tl = mine & ~head & ~ended & (rk[:, 2:] == key).any(axis=1)
        hit |= tl
        walk &= ~tl
    return hit


def predicate(sim, entries, tm):
    """(holds [entries][N] — for every node, running or not — and the running mask [N]) of the state `sim` is in now.
    tm: a TrackModel of `sim` (its baselines of recycled slots)."""
    n = int(sim.cfg.n_nodes)
    up = running(sim)
    out = np.zeros((len(entries), n), bool)
    slot = view = None
    rings = {}
    for i, (kind, key, ltime) in enumerate(entries):
        if kind in (_ffi.K_JOIN, _ffi.K_LEAVE):
            if slot is None:
                slot, view, _ = tm._dumps()
            lt, _, bits = tm._entry(key, slot, view)
            out[i] = np.broadcast_to(((bits & 1) != 0) & (lt >= np.uint64(ltime)), (n,))
        else:
            which, b = (_ffi.ARR_ERING, int(sim.cfg.event_ring)) if kind == _ffi.K_EVENT else (_ffi.ARR_QRING, int(sim.cfg.query_ring))
            if which not in rings:
                rings[which] = sim.dump(which).reshape(-1, n)
            out[i] = ring_holds(rings[which], int(sim.cfg.ring_overflow), b, key, ltime)
    return out, up


def node_records(arrival, first, up):
    """Every node's record (SPREAD_NODE_DTYPE [N]) over the started entries."""
    n = arrival.shape[1]
    started = first != 0
    a = arrival[started].astype(np.int64)
    f = first[started].astype(np.int64)[:, None]
    has = a != 0
    late = np.where(has, a - f, 0)
    rec = np.zeros(n, _ffi.SPREAD_NODE_DTYPE)
    rec["id"], rec["running"] = np.arange(n), up
    rec["got"], rec["missed"] = has.sum(axis=0), (~has).sum(axis=0)
    rec["late_sum"] = late.sum(axis=0)
    rec["late_max"] = late.max(axis=0) if len(a) else 0
    return rec


class SpreadModel:
    """sim_spread_start / count / read / stop / map / summary / unreached / late on a Sim without them: step() advances one
    tick at a time and latches behind the ticks the rule of include/serf_sim_spread.h names."""

    def __init__(self, sim, on_tick=None):
        self.sim, self.on_tick = sim, on_tick
        self.tm = TrackModel(sim)
        self.running = False
        self.samples, self.dropped = [], 0

    def start(self, entries, first_tick=0, period=1, capacity=1 << 12):
        assert not self.running and period > 0 and 0 < capacity <= _ffi.SPREAD_MAX_SAMPLES
        self.entries = [tuple(int(x) for x in e) for e in entries]
        check_entries(self.sim, self.entries)
        self.first, self.period, self.capacity = max(first_tick, self.sim.tick), period, capacity
        self.arrival = np.zeros((len(self.entries), int(self.sim.cfg.n_nodes)), np.uint32)
        self.samples, self.dropped, self.running = [], 0, True

    def stop(self):
        assert self.running
        self.running = False
        self.samples, self.dropped = [], 0

    def sample(self):
        """Latches the state the handle is in now (after tick sim.tick - 1) and returns the sample's 8 + 8 n words."""
        now = self.sim.tick
        holds, up = predicate(self.sim, self.entries, self.tm)
        hit = holds & up[None, :]
        new = hit & (self.arrival == 0)
        self.arrival[new] = now
        a = self.arrival
        w = np.zeros(HW + EW * len(self.entries), np.uint64)
        reached_up = ((a != 0) & up[None, :]).sum(axis=1)
        w[0], w[1], w[2], w[3] = now, int(up.sum()), len(self.entries), int(new.sum())
        w[4] = int((a != 0).any(axis=1).sum())
        w[5] = int((reached_up == up.sum()).sum()) if up.any() else 0
        for i, (kind, key, ltime) in enumerate(self.entries):
            o = HW + EW * i
            nz = a[i][a[i] != 0]
            w[o], w[o + 1], w[o + 2], w[o + 3] = key | (kind << 32), ltime, int(new[i].sum()), len(nz)
            w[o + 4], w[o + 5] = int(reached_up[i]), int(hit[i].sum())
            w[o + 6], w[o + 7] = (int(nz.min()), int(nz.max())) if len(nz) else (0, 0)
        return w

    def after_tick(self, t):
        """Tick t has just run (by whoever steps the handle): the baselines of recycled slots, then its sample when one is due."""
        self.tm.evaluate()
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
        """(headers, records) of samples first .. first + n - 1, as Sim.spread_read returns them."""
        sel = self.samples[first:] if n is None else self.samples[first:first + n]
        return _ffi.spread_split(np.array(sel, np.uint64).reshape(-1), len(self.entries))

    # ---- the reads of the map: from the arrivals and the running flags the handle has now ----
    def map(self, entry, first_node=0, count=None):
        return self.arrival[entry][first_node:None if count is None else first_node + count].copy()

    def firsts(self):
        a = self.arrival.astype(np.int64)
        return np.where(a != 0, a, 1 << 62).min(axis=1) * (a != 0).any(axis=1)

    def summary(self, bin_width=1):
        assert bin_width > 0
        up = running(self.sim)
        out = np.zeros(len(self.entries), _ffi.SPREAD_SUMMARY_DTYPE)
        first = self.firsts()
        for i, (kind, key, ltime) in enumerate(self.entries):
            a = self.arrival[i].astype(np.int64)
            has = a != 0
            delay = a[has] - first[i]
            s = out[i]
            s["id"], s["val"], s["first"], s["last"] = key | (kind << 32), ltime, first[i], a.max()
            s["reached"], s["reached_up"], s["unreached_up"] = has.sum(), (has & up).sum(), (~has & up).sum()
            s["late_sum"] = delay.sum()
            s["bins"] = np.bincount(np.minimum(delay // bin_width, _ffi.SPREAD_BINS - 1), minlength=_ffi.SPREAD_BINS)
        return out

    def unreached(self, entry, cap=None):
        ids = np.nonzero((self.arrival[entry] == 0) & running(self.sim))[0].astype(np.uint32)
        return ids[:cap], len(ids)

    def late(self, top_k=8, rank_by=_ffi.SPREAD_BY_MISSED, nodes=False):
        every = node_records(self.arrival, self.firsts(), running(self.sim))
        top = np.zeros(top_k, _ffi.SPREAD_NODE_DTYPE)
        order = _ffi.spread_rank(every, rank_by, top_k)
        top[:len(order)] = every[order]
        return (top, every) if nodes else top
