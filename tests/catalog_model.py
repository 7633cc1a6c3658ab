"""Reference model of the rumour catalogue (include/serf_sim_catalog.h): the catalogue as a fold over the canonical dumps
(ARR_ROWS / ARR_QUEUE / ARR_INBOX) of any _ffi.Sim, written from the header's text: the live set of a state, a sample's 48
words, the registry and the sampling rule on a handle that is stepped one tick at a time.  The CPU oracle has no catalogue;
with this model it is the checker of the HIP library's.  The twin of tests/ledger_model.py, whose readers of the dumps it uses."""
import numpy as np

from serf_amd import _ffi
from tests.ledger_model import TWO_PART, queued_records, wire_records

SW, RW = _ffi.CATALOG_SAMPLE_WORDS, _ffi.CATALOG_RECORD_WORDS
LIVE, MASK48 = _ffi.CATALOG_LIVE, (1 << 48) - 1
HOLD, QUEUED, TX, FLIGHT, FRESH = range(5)


def identity(kind, key, val):
    """(id, val) of a record: SUSPECT / DEAD keep the incarnation, the other kinds the 48 bits that travel."""
    return key | (kind << 32), val & (0xFFFFFF if kind in TWO_PART else MASK48)


def live_set(sim, kinds_mask=_ffi.CATALOG_KINDS):
    """The state `sim` is in now: ({(id, val): [holders, queued, transmits, in flight, fresh]} over the kinds of the mask, in
    ascending (id, val); the header sums (running, queued, in flight, packets, transmits) over ALL kinds)."""
    node, qk, qkey, qval, qtx, up = queued_records(sim)
    wk, wkey, wval, packets = wire_records(sim)
    sums = (int(up.sum()), len(qk), len(wk), packets, int(qtx.sum()))

    def chosen(kind, key, val):
        """(id, val) rows of the records whose kind the mask has, and which those are."""
        kind = kind.astype(np.int64)
        sel = ((kinds_mask >> kind) & 1) != 0
        kind, key, val = kind[sel], key[sel].astype(np.uint64), val[sel].astype(np.uint64)
        two = (kind == TWO_PART[0]) | (kind == TWO_PART[1])
        val = np.where(two, val & np.uint64(0xFFFFFF), val & np.uint64(MASK48))
        return np.stack([key | (kind.astype(np.uint64) << np.uint64(32)), val], axis=1), sel

    qrows, qsel = chosen(qk, qkey, qval)
    wrows, _ = chosen(wk, wkey, wval)
    if not len(qrows) and not len(wrows):
        return {}, sums
    uniq, inv = np.unique(np.concatenate([qrows, wrows]), axis=0, return_inverse=True)     # ascending (id, val)
    inv = inv.reshape(-1)
    qi, wi, n = inv[:len(qrows)], inv[len(qrows):], len(uniq)
    tx = qtx[qsel].astype(np.int64)
    c = np.zeros((n, 5), np.int64)
    c[:, QUEUED] = np.bincount(qi, minlength=n)
    c[:, TX] = np.bincount(qi, weights=tx, minlength=n).astype(np.int64)
    c[:, FRESH] = np.bincount(qi[tx == 0], minlength=n)
    pairs = np.unique(np.stack([node[qsel].astype(np.int64), qi], axis=1), axis=0) if len(qi) else np.zeros((0, 2), np.int64)
    c[:, HOLD] = np.bincount(pairs[:, 1], minlength=n)                                     # a node counts once
    c[:, FLIGHT] = np.bincount(wi, minlength=n)
    return {(int(i), int(v)): c[k].tolist() for k, (i, v) in enumerate(uniq.tolist())}, sums


def live_table(found):
    """The live table as Sim.catalog_live returns it."""
    out = np.zeros(len(found), _ffi.CATALOG_LIVE_DTYPE)
    for i, ((ident, val), c) in enumerate(found.items()):
        out[i] = (ident, val, 0, c[HOLD], c[QUEUED], c[TX], c[FLIGHT], c[FRESH])
    return out


def stateless_sample(sim, kinds_mask=_ffi.CATALOG_KINDS):
    """sim_catalog_now: (the 48 words, the live table); words 4-8 and 34 are 0."""
    found, sums = live_set(sim, kinds_mask)
    w = np.zeros(SW, np.uint64)
    w[0], w[1] = sim.tick, sums[0]
    w[9:13] = sums[1:]
    if len(found) > LIVE:
        w[3] = 1
        return w, live_table({})
    w[2] = len(found)
    for (ident, _), c in found.items():
        k = ident >> 32
        w[13 + k - 1] += 1
        w[20 + k - 1] += c[QUEUED]
        w[27 + k - 1] += c[FLIGHT]
    return w, live_table(found)


class CatalogModel:
    """sim_catalog_start / count / read / list / live / now / stop on a Sim without them: step() advances one tick at a time and
    takes the samples the rule of include/serf_sim_catalog.h asks for."""

    def __init__(self, sim, on_tick=None):
        self.sim, self.on_tick = sim, on_tick
        self.running = False
        self.samples, self.dropped = [], 0

    def start(self, kinds_mask=_ffi.CATALOG_KINDS, max_ids=_ffi.CATALOG_MAX, first_tick=0, period=1, capacity=1 << 12):
        assert not self.running and period > 0 and 0 < capacity <= _ffi.CATALOG_MAX_SAMPLES
        assert kinds_mask and not kinds_mask & ~_ffi.CATALOG_KINDS and 0 < max_ids <= _ffi.CATALOG_MAX
        self.mask, self.max_ids = kinds_mask, max_ids
        self.first, self.period, self.capacity = max(first_tick, self.sim.tick), period, capacity
        self.samples, self.dropped, self.running = [], 0, True
        self.registry, self.index = [], {}      # records as lists of python ints, (id, val) -> place
        self.previous = set()                   # the live set of the latest sample that did not overflow
        self.lost = self.overflowed = 0
        self.latest = live_table({})

    def stop(self):
        assert self.running
        self.running = False
        self.samples, self.dropped = [], 0

    def take(self):
        """One sample of the state the handle is in."""
        w, table = stateless_sample(self.sim, self.mask)
        now = int(w[0])
        if w[3]:
            self.overflowed += 1
            self.latest = live_table({})
        else:
            found = {(int(r["id"]), int(r["val"])): r for r in table}
            new = died = revived = 0
            died = len(self.previous - set(found))
            for ident, r in found.items():              # (ascending)
                q, hold, fl = int(r["queued"]), int(r["holders"]), int(r["in_flight"])
                at = self.index.get(ident)
                if at is None:
                    if ident in self.previous:          # lost before and still live: counted when it appeared
                        continue
                    if len(self.registry) < self.max_ids:
                        self.index[ident] = len(self.registry)
                        self.registry.append(dict(id=ident[0], val=ident[1], first_seen=now, last_seen=now, samples=1, revivals=0,
                                                  peak_queued=q, peak_queued_at=now, peak_holders=hold, peak_holders_at=now,
                                                  in_flight_sum=fl, queued_sum=q))
                        new += 1
                    else:
                        self.lost += 1
                    continue
                rec = self.registry[at]
                rec["last_seen"] = now
                rec["samples"] += 1
                if ident not in self.previous:
                    rec["revivals"] += 1
                    revived += 1
                if q > rec["peak_queued"]:
                    rec["peak_queued"], rec["peak_queued_at"] = q, now
                if hold > rec["peak_holders"]:
                    rec["peak_holders"], rec["peak_holders_at"] = hold, now
                rec["in_flight_sum"] += fl
                rec["queued_sum"] += q
            w[4], w[5], w[6] = new, died, revived
            self.previous = set(found)
            self.latest = table
        w[7], w[8], w[34] = len(self.registry), self.lost, self.overflowed
        return w

    def after_tick(self, t):
        """Tick t has just run (by whoever steps the handle): its sample, when one is due."""
        if self.running and t >= self.first and (t - self.first) % self.period == 0:
            if len(self.samples) < self.capacity:
                self.samples.append(self.take())
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
        sel = self.samples[first:] if n is None else self.samples[first:first + n]
        return np.array(sel, np.uint64).reshape(-1, SW).view(_ffi.CATALOG_SAMPLE_DTYPE).reshape(-1)

    def list(self, first=0, n=None):
        sel = self.registry[first:] if n is None else self.registry[first:first + n]
        out = np.zeros(len(sel), _ffi.CATALOG_RECORD_DTYPE)
        for i, rec in enumerate(sel):
            out[i] = tuple(rec[name] for name in _ffi.CATALOG_RECORD_DTYPE.names)
        return out

    def live(self):
        return self.latest

    def now(self, kinds_mask=_ffi.CATALOG_KINDS):
        w, table = stateless_sample(self.sim, kinds_mask)
        return w.view(_ffi.CATALOG_SAMPLE_DTYPE)[0], table
