"""Reference model of the kRandomNodes fan-out graph (SIM_CF_RANDOM_FANOUT; serf_amd/csrc/serf_sim_kernels.inc rf_* / rfx_*): what
the build leaves in memory, row by row, from the tick's target draw alone — tests/traffic_model.py::k_random_nodes_all, itself pinned
node by node against tests/third_model.py::k_random_nodes.  The graph is a pure function of (seed, tick, N, fan-out): the pairs
p = 4 * sender + slot in a stable order by target.  Three views of it:

  one handle             rcsr[N + 1], rsrc[rcsr[N]]: row t = the pairs that drew t, p ascending (global sender ids);
  a shard's sending side the pairs of the senders g * M + c * M / C .. of shard g's chunk c (pair ids local to the shard), sorted by
                         (destination shard, local target, p); a count byte per target of every destination, the totals of the
                         buckets of 2^LB targets (NBh = ceil(M / 2^LB) per destination), where every destination's pairs start;
  a shard's receiving    row tl of shard g = the runs of the sources q = s * C + c, s ascending then c; an entry = the packet's
  side                   cell in the receive buffer, (cell0(q) + off * PG) << 2 with cell0(q) = (c * V + s) * slab_u + cell_u and
                         off = the pair's place in source q's list for destination g.

numpy only: no device, no library.  tests/test_graph_build.py checks the model, tests/test_graph_build_gpu.py the build against it."""
import functools

import numpy as np

from tests import traffic_model


@functools.lru_cache(maxsize=16)
def k_random_nodes_all(seed, tick, n, feff):
    """traffic_model.k_random_nodes_all, drawn once per (seed, tick, n, feff) and shared read-only."""
    tg = traffic_model.k_random_nodes_all(seed, tick, n, feff)
    tg.setflags(write=False)
    return tg


def feff_of(n, fanout):
    """The fan-out a tick really has: fewer other nodes than `fanout` leave slots without a target."""
    return min(fanout, n - 1)


def pairs_of(targets, first=0, base=0):
    """The drawn (pair id, target) of the senders first .. first + len(targets) - 1, whose pair ids count from sender `base`:
    flat, in (sender, slot) order — p ascending."""
    s, k = np.nonzero(targets >= 0)
    return 4 * (s + first - base) + k, targets[s, k]


def one_handle(seed, tick, n, feff):
    """(rcsr[n + 1], rsrc): the rows of a handle that holds every node."""
    p, t = pairs_of(k_random_nodes_all(seed, tick, n, feff))
    order = np.lexsort((p, t))
    rcsr = np.concatenate(([0], np.cumsum(np.bincount(t, minlength=n))))
    return rcsr.astype(np.int64), p[order].astype(np.int64)


def sending_side(seed, tick, n, feff, V, C, g, c, LB):
    """Shard g's sender chunk c: dict(rsrc, t (the sorted pairs' global targets), cntb[n], btot[V * NBh], xoff[V + 1])."""
    M = n // V
    ns = M // C
    first = g * M + c * ns
    tg = k_random_nodes_all(seed, tick, n, feff)[first:first + ns]
    p, t = pairs_of(tg, first, g * M)
    order = np.lexsort((p, t))   # (destination, local target) ascending = global target ascending
    p, t = p[order], t[order]
    nbh = (M + (1 << LB) - 1) >> LB
    h, tl = t // M, t % M
    cnt = np.bincount(t, minlength=n)
    return dict(rsrc=p.astype(np.int64), t=t.astype(np.int64), cntb=cnt.astype(np.int64),
                btot=np.bincount(h * nbh + (tl >> LB), minlength=V * nbh).astype(np.int64),
                xoff=np.concatenate(([0], np.cumsum(np.bincount(h, minlength=V)))).astype(np.int64))


def overflow_expected(totals, bcap):
    """Entries the build puts on its overflow list: what every bucket holds beyond its region."""
    return int(np.maximum(0, np.asarray(totals, np.int64) - bcap).sum())


def bucket_totals(seed, tick, n, feff, LB):
    """One handle: the pairs in every level-1 bucket of 2^LB consecutive targets."""
    rcsr, _ = one_handle(seed, tick, n, feff)
    nb = (n + (1 << LB) - 1) >> LB
    edges = np.minimum(np.arange(nb + 1, dtype=np.int64) << LB, n)
    return rcsr[edges[1:]] - rcsr[edges[:-1]]


def receiving_side(seed, tick, n, feff, V, C, g, slab_u, cell_u, PG=1):
    """(rx_rcsr[M + 1], rx_rsrc) of shard g for the packets sent during `tick`."""
    M = n // V
    rows, srcs, ents = [], [], []
    for s in range(V):
        for c in range(C):
            snd = sending_side(seed, tick, n, feff, V, C, s, c, 8)   # (the order does not depend on the bucket width)
            lo, hi = snd["xoff"][g], snd["xoff"][g + 1]
            off = np.arange(hi - lo, dtype=np.int64)
            rows.append(snd["t"][lo:hi] - g * M)
            srcs.append(np.full(hi - lo, s * C + c, np.int64))
            ents.append((((c * V + s) * slab_u + cell_u) + off * PG) << 2)
    rows, srcs, ents = np.concatenate(rows), np.concatenate(srcs), np.concatenate(ents)
    order = np.lexsort((ents, srcs, rows))
    rcsr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=M))))
    return rcsr.astype(np.int64), ents[order]


def slab_meta(seed, tick, n, feff, V, C, s, c, g, LB, cap):
    """What slab (c, g) of shard s's send buffer says next to its cells: header (packets, flag, tick), count bytes [M], totals [NBh]."""
    M = n // V
    nbh = (M + (1 << LB) - 1) >> LB
    snd = sending_side(seed, tick, n, feff, V, C, s, c, LB)
    packets = int(snd["xoff"][g + 1] - snd["xoff"][g])
    return (min(packets, cap), 0, tick & 0xFFFFFFFF), snd["cntb"][g * M:(g + 1) * M], snd["btot"][g * nbh:(g + 1) * nbh]
