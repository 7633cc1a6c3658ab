"""Reference model of the rumour tree (include/serf_sim_tree.h) on any _ffi.Sim that is stepped one tick at a time: the packets
in flight and their targets as tests/traffic_model.py::packets takes them (ARR_INBOX and the tick's target draw), the identities
of their records as tests/ledger_model.py::wire_records reads them (kind, key, 48 value bits), the latch's predicate from
tests/spread_model.py — and the rules of the header applied with numpy: candidates, the stamp, the latch, orphans, hops.  The CPU
oracle has no tree; with this model it is the checker of the HIP library's.  The twin of tests/traffic_model.py.

tests/test_tree.py checks the model against routes that do not share its code: the spread map's arrivals, the ledger's copies,
the kRandomNodes draw of the parent, the traffic meter's tx_packets."""
import numpy as np

from serf_amd import _ffi
from tests import spread_model, traffic_model
from tests.track_model import TrackModel

HW, EW = _ffi.TREE_HEADER_WORDS, _ffi.TREE_ENTRY_WORDS
NONE = _ffi.TREE_NONE
BINS = _ffi.TREE_BINS


def carriers(sim, entries):
    """The packets in flight of the state `sim` is in now: (sender, target, carries [packets][entries] — whether a record of
    the packet, on any page, has the entry's identity —, copies [entries] — the records with it over all packets —, the
    running mask).  The packets are traffic_model.packets', in its order."""
    n, fanout = int(sim.cfg.n_nodes), int(sim.cfg.fanout)
    sender, target, rec, _, up = traffic_model.packets(sim)
    carries = np.zeros((len(sender), len(entries)), bool)
    copies = np.zeros(len(entries), np.int64)
    if not len(sender):
        return sender, target, carries, copies, up
    inbox = sim.dump(_ffi.ARR_INBOX).reshape(-1, n)                                  # [fanout * pg][cell] pages of 4 records
    pg = inbox.shape[0] // fanout
    hm = inbox["hi_meta"].astype(np.int64).reshape(fanout, pg, n, 4)
    kind = (hm >> 4) & 0xF
    key = inbox["key"].astype(np.int64).reshape(fanout, pg, n, 4)
    val = inbox["val_lo"].astype(np.int64).reshape(fanout, pg, n, 4) | ((hm >> 16) << 32)
    slot, cell = np.nonzero((kind != 0).sum(axis=(1, 3)) > 0)                         # traffic_model.packets' order
    assert len(slot) == len(sender) and ((kind != 0).sum(axis=(1, 3))[slot, cell] == rec).all()
    for i, (k, ky, lt) in enumerate(entries):
        match = (kind == k) & (key == ky) & (val == lt)                                # [fanout][pg][cell][4]
        per = match.sum(axis=(1, 3))[slot, cell]
        carries[:, i] = per > 0
        copies[i] = per.sum()
    return sender, target, carries, copies, up


class TreeModel:
    """sim_tree_start / count / read / stop / links / summary / path / top on a Sim without them: step() advances one tick at a
    time and applies the rules of include/serf_sim_tree.h behind every tick from first_tick on."""

    def __init__(self, sim, on_tick=None):
        self.sim, self.on_tick = sim, on_tick
        self.tm = TrackModel(sim)
        self.running = False
        self.samples, self.dropped = [], 0

    def start(self, entries, first_tick=0, capacity=1 << 12):
        assert not self.running and 0 < capacity <= _ffi.TREE_MAX_SAMPLES
        self.entries = [tuple(int(x) for x in e) for e in entries]
        spread_model.check_entries(self.sim, self.entries)
        self.first, self.capacity = max(first_tick, self.sim.tick), capacity
        shape = (len(self.entries), int(self.sim.cfg.n_nodes))
        self.arrival, self.hop = np.zeros(shape, np.uint32), np.zeros(shape, np.uint32)
        self.parent = np.full(shape, NONE, np.uint32)
        self.cand, self.stamp = np.full(shape, -1, np.int64), None
        self.multi = 0                                    # arrivals whose candidate was chosen among two or more different senders
        self.cand_senders = np.zeros(shape, np.int64)
        self.samples, self.dropped, self.running = [], 0, True

    def stop(self):
        assert self.running
        self.running = False
        self.samples, self.dropped = [], 0

    def sample(self):
        """Latches the state the handle is in now (after tick sim.tick - 1), computes the candidates of the packets in flight
        and returns the sample's 8 + 8 n words."""
        now, ne = self.sim.tick, len(self.entries)
        holds, up = spread_model.predicate(self.sim, self.entries, self.tm)
        latch = holds & up[None, :] & (self.arrival == 0)
        before = self.arrival.copy()
        cand = self.cand if self.stamp == now - 1 else np.full(self.cand.shape, -1, np.int64)
        has = latch & (cand >= 0)
        at = np.where(has, cand, 0)
        has &= np.take_along_axis(before, at, axis=1) != 0
        self.arrival[latch] = now
        self.parent[latch] = np.where(has, cand, NONE).astype(np.uint32)[latch]
        self.hop[latch] = np.where(has, np.take_along_axis(self.hop, at, axis=1) + 1, 0).astype(np.uint32)[latch]
        self.multi += int((has & (self.cand_senders > 1)).sum()) if self.stamp == now - 1 else 0
        orphan = latch & ~has
        # ---- after the latch: the candidates of the packets now in flight ----
        sender, target, carries, copies, _ = carriers(self.sim, self.entries)
        self.cand = np.full(self.cand.shape, -1, np.int64)
        self.cand_senders = np.zeros(self.cand.shape, np.int64)
        fresh = np.zeros(ne, np.int64)
        big = np.iinfo(np.int64).max
        for i in range(ne):
            sel = carries[:, i] & (self.arrival[i][target] == 0) if len(target) else np.zeros(0, bool)
            fresh[i] = int((sel & up[target]).sum()) if len(target) else 0
            if sel.any():
                c = np.full(self.cand.shape[1], big, np.int64)
                np.minimum.at(c, target[sel], sender[sel])
                self.cand[i] = np.where(c == big, -1, c)
                pairs = np.unique(np.stack([target[sel], sender[sel]]), axis=1)
                self.cand_senders[i] = np.bincount(pairs[0], minlength=self.cand.shape[1])
        self.stamp = now
        w = np.zeros(HW + EW * ne, np.uint64)
        w[0], w[1], w[2], w[3], w[4] = now, int(up.sum()), ne, int(latch.sum()), int(orphan.sum())
        w[5], w[6] = int(copies.sum()), int(fresh.sum())
        for i, (kind, key, ltime) in enumerate(self.entries):
            o = HW + EW * i
            got = self.arrival[i] != 0
            w[o], w[o + 1], w[o + 2], w[o + 3] = key | (kind << 32), ltime, int(latch[i].sum()), int(orphan[i].sum())
            w[o + 4], w[o + 5] = int(got.sum()), int((got & (self.parent[i] == NONE)).sum())
            w[o + 6], w[o + 7] = int(copies[i]), int(fresh[i])
        return w

    def after_tick(self, t):
        """Tick t has just run (by whoever steps the handle): the baselines of recycled slots, then its sample when one is due."""
        self.tm.evaluate()
        if self.running and t >= self.first:
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
        """(headers, records) of samples first .. first + n - 1, as Sim.tree_read returns them."""
        sel = self.samples[first:] if n is None else self.samples[first:first + n]
        return _ffi.tree_split(np.array(sel, np.uint64).reshape(-1), len(self.entries))

    # ---- the reads ----
    def children(self, entry):
        par = self.parent[entry][(self.arrival[entry] != 0) & (self.parent[entry] != NONE)]
        return np.bincount(par.astype(np.int64), minlength=self.arrival.shape[1]).astype(np.uint32)

    def links(self, entry, first_node=0, count=None):
        out = np.zeros(self.arrival.shape[1], _ffi.TREE_LINK_DTYPE)
        got = self.arrival[entry] != 0
        out["arrival"], out["hop"], out["children"] = self.arrival[entry], self.hop[entry], self.children(entry)
        out["parent"] = np.where(got, self.parent[entry], NONE)
        return out[first_node:None if count is None else first_node + count].copy()

    def summary(self):
        out = np.zeros(len(self.entries), _ffi.TREE_SUMMARY_DTYPE)
        for i, (kind, key, ltime) in enumerate(self.entries):
            lk = self.links(i)
            ids = np.nonzero(lk["arrival"] != 0)[0]
            got = lk[ids]
            s = out[i]
            s["id"], s["val"], s["reached"], s["orphans"] = key | (kind << 32), ltime, len(got), int((got["parent"] == NONE).sum())
            if len(got):
                ch = got["children"].astype(np.int64)
                s["depth"], s["hop_sum"] = got["hop"].max(), got["hop"].astype(np.int64).sum()
                s["most_children"], s["most_children_id"] = ch.max(), ids[np.argmax(ch)]   # (argmax: the first = the smallest id)
                s["hop_bins"] = np.bincount(np.minimum(got["hop"].astype(np.int64), BINS - 1), minlength=BINS)
                s["children_bins"] = np.bincount(np.minimum(ch, BINS - 1), minlength=BINS)
        return out

    def path(self, entry, node, cap=None):
        ids = []
        if self.arrival[entry][node]:
            at = node
            while True:
                ids.append(at)
                if self.parent[entry][at] == NONE:
                    break
                at = int(self.parent[entry][at])
        return np.array(ids[:cap], np.uint32), len(ids)

    def top(self, entry, top_k=10):
        lk = self.links(entry)
        n = len(lk)
        order = np.lexsort((np.arange(n), -lk["children"].astype(np.int64)))[:top_k]
        up = spread_model.running(self.sim)
        top = np.zeros(top_k, _ffi.TREE_RANK_DTYPE)
        top["id"] = 0xFFFFFFFF
        top["id"][:len(order)] = order
        top["running"][:len(order)] = up[order]
        top["link"][:len(order)] = lk[order]
        return top
