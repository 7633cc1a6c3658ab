/*
 * serf_sim_tree.h — rumour tree on the device: for a fixed set of record identities, who infected whom — per node the tick it
 * first had the rumour, the node whose packet brought it, and its hop count from the origin —, latched behind every tick,
 * without a host poll.
 *
 * The ninth extension of include/serf_sim.h, in the style of include/serf_sim_spread.h and include/serf_sim_traffic.h:
 * exported by the HIP library (libserf_sim.so) only, with a version of its own (sim_tree_version), not part of
 * SIM_ABI_VERSION.  The CPU oracle has no tree: it is the checker — every word below is a pure function of the arrays the
 * oracle dumps (SIM_ARR_INBOX and the arrays of include/serf_sim_spread.h) and of the tick's target draw (tests/tree_model.py).
 *
 * The spread map says when each node got a rumour, the traffic meter how the packets load each node, the ledger how many
 * copies travel.  The tree joins them: the epidemic tree of a rumour and its hop-count distribution (the depth that
 * retransmit_mult * log N is meant to bound), how many nodes each node was the first to tell, how many of the copies in flight
 * are still useful, the chain by which a late node finally got the rumour.  A tree adds no protocol state: digests, events,
 * dumps, checkpoint images do not know it, and a handle without a started tree launches, allocates and synchronises nothing
 * for it.
 *
 * ENTRIES.  An entry is the spread map's: kind SIM_K_JOIN .. SIM_K_QUERY (1-4), key (JOIN / LEAVE: the subject, < n_nodes;
 * EVENT / QUERY: the event key or query id, non-zero), ltime < 2^48; 64 entries at most, fixed for the tree's life.  The
 * struct is sim_spread_entry.
 *
 * SAMPLING.  The period is 1 and is not an argument: a parent is found from the packets of the tick before.
 *
 * CARRIER.  A carrier of entry e behind tick t is a packet of that sample as include/serf_sim_traffic.h defines one — a
 * (sender, fan-out slot) with a non-empty record, all pages together, with the target that header names — of which at least
 * one record has the identity (kind, key, 48 value bits) of e: the ledger's match for kinds 1-4.  Packets that loss or
 * gossip_to_the_dead zeroed are not seen.
 *
 * CANDIDATE.  cand[e][l] is the smallest sender id among the carriers of e addressed to l.  Candidates carry the `now` they
 * were computed at.
 *
 * LATCH.  Behind tick t (now = t + 1), for every running node l with arrival[e][l] == 0 for which the predicate of
 * sim_convergence holds:
 *   - arrival[e][l] = now.  This is exactly the spread map's plane.
 *   - Let p be the candidate computed by the sample behind tick t - 1.  It is used only if that sample was taken and its
 *     stamp equals now - 1.
 *   - If there is no such candidate, or arrival[e][p] before this sample was 0, then parent = 0xFFFFFFFF and hop = 0.  This is
 *     an ORPHAN: the origin, a push-pull, a superseding JOIN / LEAVE record, a holder from before the first sample, or the
 *     first sample after a restore.  (On the device the parent's arrival is read as a != 0 && a < now, so that a parent
 *     latching in the same launch cannot matter.)
 *   - Otherwise parent = p and hop = hop[e][p] + 1.
 *   - Nothing is ever cleared.  A crash, a revive, a recycled slot and a reused bucket leave the record alone.
 *
 * RESTORE.  sim_snapshot holds no tree, sim_restore leaves a running one as it is.  The stamp rule makes the first sample
 * after a restore latch orphans.
 *
 * AFTER THE LATCH the sample computes the candidates of the packets now in flight, stamps them `now`, and computes its words.
 * A sample that is due with the buffer full is dropped and counted: it latches nothing and computes no candidates, so the
 * tree stops growing — give the buffer the room the run needs.
 *
 * Out of scope: sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED) — every call below returns SIM_ESTATE on such a
 * handle (vshards > 1 on a handle that holds every node is one handle and is supported).  Both fan-out models are supported.
 */
#ifndef SERF_SIM_TREE_H
#define SERF_SIM_TREE_H

#include <stddef.h>

#include "serf_sim.h"
#include "serf_sim_spread.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_TREE_VERSION 1u
#define SIM_TREE_MAX 64u                 /* entries per tree (= SIM_SPREAD_MAX) */
#define SIM_TREE_MAX_SAMPLES (1u << 20)
#define SIM_TREE_HEADER_WORDS 8u
#define SIM_TREE_ENTRY_WORDS 8u
#define SIM_TREE_BINS 32u                /* bins of either histogram of sim_tree_summary */
#define SIM_TREE_SUMMARY_WORDS (8u + 2u * SIM_TREE_BINS)
#define SIM_TREE_TOP_MAX 64u
#define SIM_TREE_NONE 0xFFFFFFFFu        /* the parent of an orphan and of a node without an arrival */

typedef sim_spread_entry sim_tree_entry; /* 16 bytes: { kind, key, ltime } */

/* One node's place in one entry's tree.  A node without an arrival: { 0, SIM_TREE_NONE, 0, children = 0 }. */
typedef struct sim_tree_link {
  uint32_t arrival;   /* the spread map's: now of the sample that latched the node, 0 = not yet */
  uint32_t parent;    /* SIM_TREE_NONE: an orphan */
  uint32_t hop;       /* 0 for an orphan, hop[parent] + 1 otherwise */
  uint32_t children;  /* the nodes whose parent it is, counted by the read */
} sim_tree_link;                                                                                        /* 16 bytes */
typedef struct sim_tree_rank { uint32_t id; uint32_t running; sim_tree_link link; } sim_tree_rank;      /* 24 bytes */

/* A sample = 8 + 8 n unsigned 64-bit words: a header, then 8 words per entry, in the order the entries were given.  All
 * words are integers and describe the state AFTER the sampled tick (what the dumps show when sim_tick == t + 1).
 *
 * Header:
 *   0   now: sim_tick after the tick (t + 1)
 *   1   running nodes
 *   2   n
 *   3   arrivals latched by this sample, over all entries
 *   4   of them orphans
 *   5   matching records in flight, over all entries
 *   6   fresh carriers, over all entries
 *   7   0
 * Entry i, words 8 + 8 i ..:
 *   0   id: key | (uint64_t)kind << 32
 *   1   val: the ltime
 *   2   new: arrivals latched by this sample
 *   3   new orphans: of them orphans
 *   4   reached: nodes with an arrival so far
 *   5   orphans so far
 *   6   copies: records in flight with the entry's identity — by definition the ledger's word 6 of the same state
 *   7   fresh: carriers addressed to a running node that has no arrival yet
 *
 * Errors of all calls: SIM_EINVAL for null pointers, n == 0 or > SIM_TREE_MAX, an entry of a kind outside 1-4, a key out of
 * range, an ltime >= 2^48, two equal entries, capacity == 0 or > SIM_TREE_MAX_SAMPLES, a read beyond `taken` (or into a
 * buffer that is too small), an entry >= n, nodes beyond n_nodes, top_k == 0 or > SIM_TREE_TOP_MAX; SIM_ESTATE on a sharded
 * handle, between sim_step_begin and sim_step_end, for a start while a tree is running and for a read / stop without one;
 * SIM_ENOMEM when the planes (n_nodes * (12 n + 48) bytes), the sample buffer or a read's scratch cannot be allocated.  Bad
 * arguments are SIM_EINVAL before "no tree" / "already running" is SIM_ESTATE (an entry >= n needs the tree: it comes behind
 * "no tree").  A call that fails changes nothing. */

/* A sample is taken behind every tick t >= first_tick until `capacity` samples are held.  A first_tick that has passed
 * already means "now" (the handle's tick).  The planes start at zero: whoever holds a rumour at the first sample is latched
 * there as an orphan. */
int sim_tree_start(sim_handle*, const sim_tree_entry* entries, uint32_t n, uint32_t first_tick, uint32_t capacity);
/* Samples taken / dropped so far: the host knows every sampled tick in advance, so this waits for nothing.  Both are 0 on a
 * handle without a tree. */
int sim_tree_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken) into out[cap_words]
 * (n * (8 + 8 entries) <= cap_words); *n_out = n. */
int sim_tree_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Frees the planes and the samples. */
int sim_tree_stop(sim_handle*);

/* The reads.  Each waits for the handle's stream, computes on the device on scratch of its own, and leaves the tree
 * untouched. */

/* The links of nodes first_node .. first_node + count - 1 of one entry into out[count] (first_node + count <= n_nodes). */
int sim_tree_links(sim_handle*, uint32_t entry, uint32_t first_node, uint32_t count, sim_tree_link* out);
/* Per entry SIM_TREE_SUMMARY_WORDS (8 + 32 + 32) words, out[n][72]:
 *   0   id                              1   val
 *   2   reached                         3   orphans
 *   4   depth: the largest hop          5   the sum of the hops
 *   6   the most children of a reached node     7   the smallest id that has them; 6 and 7 are 0 while nobody is reached
 *   8 + b    reached nodes with min(hop, 31) == b
 *   40 + b   reached nodes with min(children, 31) == b */
int sim_tree_summary(sim_handle*, uint64_t* out);
/* The chain node, parent, grandparent ... up to its orphan: *total = hop + 1 ids (0 for a node without an arrival), the first
 * min(cap, *total) of them in ids[], *n_out of them.  ids may be null when cap is 0. */
int sim_tree_path(sim_handle*, uint32_t entry, uint32_t node, uint32_t* ids, uint32_t cap, uint32_t* n_out, uint32_t* total);
/* ranks[top_k]: ALL nodes of one entry ranked by children descending, ties by ascending id; `running` is the node's flag
 * now.  Records beyond n_nodes carry id 0xFFFFFFFF and zeros. */
int sim_tree_top(sim_handle*, uint32_t entry, uint32_t top_k /* 1 .. 64 */, sim_tree_rank* ranks);
uint32_t sim_tree_version(void);

#ifdef __cplusplus
}
#endif
#endif
