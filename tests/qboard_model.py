"""Reference model of the query board (include/serf_sim_qboard.h): every word of a sample and every read, as a pure function of
what any _ffi.Sim gives behind a tick —

  query_status / query_responders per id   acks, responses, the bitmaps, `open`; a refusal means the id does not own its table entry
  the ARR_ROWS dump                        who runs (SIM_RF_UP)
  the script's own operations              the filter records and the tag classes: the model is handed every operation the script
                                           schedules (Script below) and replays SIM_OP_QUERY_FILTER_ID / _TAGS / SIM_OP_QUERY /
                                           SIM_OP_SET_TAGS and init_tags as the host path does — a record is started by the first
                                           operation that names the query, sealed by its SIM_OP_QUERY, taken over by another id of the
                                           same residue; a SIM_OP_SET_TAGS stores the class whether or not the node runs.  Origin,
                                           flags and deadline of a query are those of its SIM_OP_QUERY (deadline = its tick + the
                                           query timeout): tests/test_qboard.py compares them with the image's running-query section

The CPU oracle has no board; with this model it is the checker of the HIP library's.  The twin of tests/spread_model.py."""
import numpy as np

from serf_amd import _ffi

HW, EW = _ffi.QBOARD_HEADER_WORDS, _ffi.QBOARD_ENTRY_WORDS
RF_UP = 1
SIM_QT, QF_IDS = 256, 12                         # include/serf_sim.h: running-query table entries, ids a filter record holds
WAITING, OPEN, CLOSED, DISPLACED = _ffi.QBOARD_WAITING, _ffi.QBOARD_OPEN, _ffi.QBOARD_CLOSED, _ffi.QBOARD_DISPLACED
FILTER_OPS = (_ffi.OP_QUERY_FILTER_ID, _ffi.OP_QUERY_FILTER_TAGS, _ffi.OP_QUERY)


def q_timeout(n):
    """query.rs:421-427 with query_timeout_mult = 16: sixteen ticks per decimal digit of the cluster size."""
    return 16 * len(str(n))


def running(sim):
    return (sim.dump(_ffi.ARR_ROWS)["flags"].astype(np.int64) & RF_UP) != 0


class Script:
    """What a scenario schedules, kept for the model: the same calls go to every Sim handed in (the oracle, the HIP handle).  A
    scenario is a function of a Script-like object — anything with inject / init_tags — so it runs on a bare Sim as well."""

    def __init__(self, *sims):
        self.sims = sims
        self.ops = []                             # (tick as scheduled, op, node, a, b), in schedule order
        self.tags0 = None

    def inject(self, tick, op, node, a=0, b=0):
        for s in self.sims:
            s.inject(tick, op, node, a, b)
        self.ops.append((max(int(tick), int(self.sims[0].tick)) if self.sims else int(tick), op, node, a, b))

    def init_tags(self, classes, first=0):
        for s in self.sims:
            s.init_tags(classes, first)
        assert first == 0 and self.tags0 is None
        self.tags0 = np.asarray(classes, np.uint8).copy()

    def query(self, tick, node, qid, flags, ids=None, mask=_ffi.NO_TAG_FILTER):
        """sim_query_filtered as operations: the ids, the mask, then the query itself."""
        for x in ids or ():
            self.inject(tick, _ffi.OP_QUERY_FILTER_ID, node, qid, x)
        if mask != _ffi.NO_TAG_FILTER:
            self.inject(tick, _ffi.OP_QUERY_FILTER_TAGS, node, qid, mask)
        self.inject(tick, _ffi.OP_QUERY, node, qid, flags)


class Tables:
    """The running-query table, the filter records and the tag classes as the operations up to a tick leave them."""

    def __init__(self, n):
        self.n = n
        self.qt = {}                              # residue -> (id, origin, deadline, flags)
        self.filt = {}                            # residue -> dict(id, ids, mask, sealed)
        self.tags = np.zeros(n, np.int64)
        self.done = 0                             # operations of the script replayed so far

    def replay(self, script, now):
        """The operations scheduled for ticks below `now`, in schedule order within a tick (sim_inject keeps it)."""
        if script.tags0 is not None and self.done == 0:
            self.tags[:len(script.tags0)] = script.tags0
        ops = sorted(enumerate(script.ops), key=lambda x: (x[1][0], x[0]))
        for k in range(self.done, len(ops)):
            _, (tick, op, node, a, b) = ops[k]
            if tick >= now:
                assert all(o[1][0] >= now for o in ops[k:])
                break
            self.done = k + 1
            if op == _ffi.OP_SET_TAGS:
                self.tags[node] = a
            if op not in FILTER_OPS:
                continue
            f = self.filt.get(a % SIM_QT)
            if f is None or f["id"] != a or f["sealed"]:          # (op_query_filter, serf_sim_step.inc)
                f = self.filt[a % SIM_QT] = dict(id=a, ids=[], mask=0xFFFFFFFF, sealed=False)
            if op == _ffi.OP_QUERY_FILTER_ID:
                if len(f["ids"]) < QF_IDS:                          # (a 13th id is dropped and counted)
                    f["ids"].append(b)
            elif op == _ffi.OP_QUERY_FILTER_TAGS:
                f["mask"] &= b
            else:
                f["sealed"] = True
                self.qt[a % SIM_QT] = (a, node, (tick + q_timeout(self.n)) & 0xFFFFFFFF, b)

    def owner(self, qid):
        t = self.qt.get(qid % SIM_QT)
        return t if t and t[0] == qid else None

    def admitted(self, qid):
        """query_should_process for every node, against the filter record and the tag classes as they are now."""
        f = self.filt.get(qid % SIM_QT)
        out = np.ones(self.n, bool)
        if f is None or f["id"] != qid:
            return out                                            # no filters on record for this query
        if f["mask"] != 0xFFFFFFFF:
            out &= ((f["mask"] >> self.tags) & 1) != 0
        if f["ids"]:
            out &= np.isin(np.arange(self.n), f["ids"])
        return out


def bitmaps(sim, qid):
    """(ack bits, response bits) [N] of a query that owns its entry, through sim_query_responders."""
    n = int(sim.cfg.n_nodes)
    out = np.zeros((2, n), bool)
    for which in (0, 1):
        out[which][sim.query_responders(qid, which)] = True
    return out


def state_of(sim, tab, ids):
    """What a sample reads, per id: None when the id does not own its entry, else dict(origin, flags, deadline, open, ack, rsp,
    adm) — the refusal of query_status and the table replayed from the operations have to agree."""
    out = []
    for qid in ids:
        own = tab.owner(qid)
        try:
            acks, resp, is_open = sim.query_status(qid)
        except _ffi.SimError:
            assert own is None, f"query {qid}: the operations say it owns its entry, query_status refuses it"
            out.append(None)
            continue
        assert own is not None, f"query {qid}: query_status knows it, the operations do not"
        ack, rsp = bitmaps(sim, qid)
        assert int(ack.sum()) == acks and int(rsp.sum()) == resp
        assert is_open == (sim.tick & 0xFFFFFFFF <= own[2]), f"query {qid}: open {is_open}, deadline {own[2]}, tick {sim.tick}"
        out.append(dict(origin=own[1], deadline=own[2], flags=own[3], open=is_open, acks=acks, responses=resp, ack=ack, rsp=rsp,
                        adm=tab.admitted(qid)))
    return out


def entry_words(qid, st, up, now, prev, stateless=False):
    """One entry's 16 words from what state_of gives and the entry's previous words (zeros: waiting)."""
    w = np.array(prev, np.uint64)
    was = int(w[0]) >> 32
    if st is None:
        state = WAITING if was == WAITING else DISPLACED
        w[3:11] = 0
    else:
        origin = st["origin"] | (st["flags"] << 32)
        again = was in (WAITING, DISPLACED) or int(w[1]) != origin or int(w[2]) != st["deadline"]
        pa, pr = (0, 0) if again else (int(w[3]), int(w[4]))
        if again:
            w[11:16] = 0
        el_mask = up & st["adm"]
        el, a, r = int(el_mask.sum()), int((el_mask & st["ack"]).sum()), int((el_mask & st["rsp"]).sum())
        state = OPEN if st["open"] else CLOSED
        w[1], w[2], w[3], w[4] = origin, st["deadline"], st["acks"], st["responses"]
        w[5], w[6], w[7], w[8] = el, a, r, el - a
        w[9], w[10] = (0, 0) if stateless else (st["acks"] - pa, st["responses"] - pr)
        if not stateless and st["open"] and el:
            for k, hit in enumerate((a >= 1, 2 * a >= el, 10 * a >= 9 * el, 100 * a >= 99 * el, a == el)):
                if hit and not w[11 + k]:
                    w[11 + k] = now
    w[0] = qid | (state << 32)
    return w


def sample_words(sim, tab, ids, prev=None):
    """A sample's 8 + 16 n words of the state `sim` is in; prev: [n][16] previous words (updated in place), None: stateless."""
    now = int(sim.tick)
    up = running(sim)
    sts = state_of(sim, tab, ids)
    w = np.zeros(HW + EW * len(ids), np.uint64)
    zero = np.zeros(EW, np.uint64)
    for i, (qid, st) in enumerate(zip(ids, sts)):
        ew = entry_words(qid, st, up, now, zero if prev is None else prev[i], stateless=prev is None)
        if prev is not None:
            prev[i] = ew
        w[HW + EW * i:HW + EW * (i + 1)] = ew
    states = [int(w[HW + EW * i]) >> 32 for i in range(len(ids))]
    w[0], w[1], w[2] = now, int(up.sum()), len(ids)
    w[3], w[4], w[5], w[6] = (states.count(s) for s in (OPEN, CLOSED, WAITING, DISPLACED))
    w[7] = sum(int(w[HW + EW * i + 9]) + int(w[HW + EW * i + 10]) for i in range(len(ids)))
    return w


def node_records(sim, tab, ids):
    """Every node's record (QBOARD_NODE_DTYPE [N]) over the entries that own their table entry now."""
    n = int(sim.cfg.n_nodes)
    rec = np.zeros(n, _ffi.QBOARD_NODE_DTYPE)
    rec["id"], rec["running"] = np.arange(n), running(sim)
    for st in state_of(sim, tab, ids):
        if st is None:
            continue
        rec["asked"] += st["adm"]
        rec["acked"] += st["ack"]
        rec["responded"] += st["rsp"]
        if st["flags"] & _ffi.F_ACK:
            rec["silent_ack"] += st["adm"] & ~st["ack"]
        if st["flags"] & _ffi.F_RESPOND:
            rec["silent_resp"] += st["adm"] & ~st["rsp"]
    return rec


class QBoardModel:
    """sim_qboard_start / count / read / stop / now / silent / nodes / top on a Sim without them: step() advances one tick at a
    time and samples behind the ticks the rule of include/serf_sim_qboard.h names.  script: the Script the scenario fills."""

    def __init__(self, sim, script, on_tick=None):
        self.sim, self.script, self.on_tick = sim, script, on_tick
        self.tab = Tables(int(sim.cfg.n_nodes))
        self.running = False
        self.samples, self.dropped = [], 0

    def tables(self):
        self.tab.replay(self.script, int(self.sim.tick))
        return self.tab

    def start(self, ids, first_tick=0, period=1, capacity=1 << 12):
        assert not self.running and period > 0 and 0 < capacity <= _ffi.QBOARD_MAX_SAMPLES
        self.ids = [int(x) for x in ids]
        assert 1 <= len(self.ids) <= _ffi.QBOARD_MAX and len(set(self.ids)) == len(self.ids) and all(self.ids)
        self.first, self.period, self.capacity = max(first_tick, self.sim.tick), period, capacity
        self.prev = np.zeros((len(self.ids), EW), np.uint64)
        self.samples, self.dropped, self.running = [], 0, True

    def stop(self):
        assert self.running
        self.running = False
        self.samples, self.dropped = [], 0

    def after_tick(self, t):
        if self.running and t >= self.first and (t - self.first) % self.period == 0:
            if len(self.samples) < self.capacity:
                self.samples.append(sample_words(self.sim, self.tables(), self.ids, self.prev))
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
        """(headers, records) of samples first .. first + n - 1, as Sim.qboard_read returns them."""
        sel = self.samples[first:] if n is None else self.samples[first:first + n]
        return _ffi.qboard_split(np.array(sel, np.uint64).reshape(-1), len(self.ids))

    def now(self, ids):
        hdr, rec = _ffi.qboard_split(sample_words(self.sim, self.tables(), [int(x) for x in ids]), len(ids))
        return hdr[0], rec[0]

    # ---- the reads: from the state the handle is in now ----
    def silent(self, entry, which=0, cap=None):
        st = state_of(self.sim, self.tables(), [self.ids[entry]])[0]
        if st is None:
            return np.zeros(0, np.uint32), 0
        ids = np.nonzero(running(self.sim) & st["adm"] & ~(st["rsp"] if which else st["ack"]))[0].astype(np.uint32)
        return ids[:cap], len(ids)

    def nodes(self, first_node=0, count=None):
        return node_records(self.sim, self.tables(), self.ids)[first_node:None if count is None else first_node + count]

    def top(self, top_k=8, rank_by=_ffi.QBOARD_BY_SILENT_ACK, nodes=False):
        every = node_records(self.sim, self.tables(), self.ids)
        top = np.zeros(top_k, _ffi.QBOARD_NODE_DTYPE)
        order = _ffi.qboard_rank(every, rank_by, top_k)
        top[:len(order)] = every[order]
        return (top, every) if nodes else top
