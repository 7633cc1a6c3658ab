/*
 * serf_sim_spread.h — spread map on the device: for a fixed set of record identities, the tick at which each node first had
 * applied each of them, latched behind the sampled ticks, without a host poll.
 *
 * The seventh extension of include/serf_sim.h, in the style of include/serf_sim_ledger.h and include/serf_sim_detect.h:
 * exported by the HIP library (libserf_sim.so) only, with a version of its own (sim_spread_version), not part of
 * SIM_ABI_VERSION.  The CPU oracle has no spread map: it is the checker — every word below is a pure function of the arrays
 * the oracle dumps (SIM_ARR_ROWS / SIM_ARR_VIEW / SIM_ARR_SLOTMAP / SIM_ARR_ERING / SIM_ARR_QRING; tests/spread_model.py).
 *
 * The trackers give a rumour's 50 / 90 / 99 / 100 % latches, the ledger its reach curve and what it costs.  The map says
 * WHICH nodes got it late or never, and when each node got it: the latency distribution over the nodes, the names of the
 * unreached, a ranking of the nodes that are always last.  A map adds no protocol state: digests, events, dumps, checkpoint
 * images do not know it, and a handle without a started map launches, allocates and synchronises nothing for it.
 *
 * Checkpoints: sim_snapshot holds no map, sim_restore leaves a running one as it is — its arrivals, its first tick and its
 * period, in absolute ticks (the wording of include/serf_sim_ledger.h).
 *
 * An ENTRY names a record identity of the four kinds the reach predicate knows:
 *   kind   SIM_K_JOIN, SIM_K_LEAVE, SIM_K_EVENT, SIM_K_QUERY (1-4); kinds 5-7 are SIM_EINVAL (follow those with a
 *          SIM_TRK_MEMBER tracker or the detection log)
 *   key    JOIN / LEAVE: the subject (< n_nodes); EVENT / QUERY: the event key or query id, non-zero
 *   ltime  the Lamport time, below 2^48
 * The set of entries is fixed for the map's life: stop and start to change it.
 *
 * THE MAP: arrival[e][l], a uint32_t per entry e and node l, 0 = not yet.  Behind a sampled tick t (now = t + 1) every node l
 * is tested: if l is running (SIM_RF_UP), arrival[e][l] == 0 and the predicate of sim_convergence holds for (e, l), then
 * arrival[e][l] = now.  An arrival is never cleared while the map runs: it survives a crash, a revive, a recycled view slot
 * and a reused ring bucket.  A node that had the rumour before the first sample is latched at the first sample.  With a
 * period above 1 an arrival is the first SAMPLED tick at which the node had it.
 *
 * Out of scope: sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED) — every call below returns SIM_ESTATE on such a
 * handle (vshards > 1 on a handle that holds every node is one handle and is supported); who infected whom (that is include/serf_sim_tree.h).
 */
#ifndef SERF_SIM_SPREAD_H
#define SERF_SIM_SPREAD_H

#include <stddef.h>

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_SPREAD_VERSION 1u
#define SIM_SPREAD_MAX 64u            /* entries per map (= SIM_CONV_MAX) */
#define SIM_SPREAD_MAX_SAMPLES (1u << 20)
#define SIM_SPREAD_HEADER_WORDS 8u
#define SIM_SPREAD_ENTRY_WORDS 8u
#define SIM_SPREAD_BINS 32u           /* histogram bins of sim_spread_summary */
#define SIM_SPREAD_SUMMARY_WORDS (8u + SIM_SPREAD_BINS)
#define SIM_SPREAD_TOP_MAX 64u
#define SIM_SPREAD_NODE_WORDS 8u

/* what sim_spread_late ranks the running nodes by */
#define SIM_SPREAD_BY_MISSED 0u       /* (missed descending, late_sum descending, id ascending) */
#define SIM_SPREAD_BY_LATE 1u         /* (late_sum descending, missed descending, id ascending) */

typedef struct sim_spread_entry { uint32_t kind; uint32_t key; uint64_t ltime; } sim_spread_entry;   /* 16 bytes: sim_ledger_entry's layout */

/* One node's record over the STARTED entries (those with first != 0: somebody has an arrival):
 *   0   id | (uint64_t)running << 32      (running: whether the node runs now)
 *   1   got: entries the node has an arrival for
 *   2   missed: started entries it has none for
 *   3   late_sum: the sum of arrival - first[e] over the entries of word 1
 *   4   late_max: the largest of them
 *   5-7 0 */
typedef struct sim_spread_node { uint64_t w[SIM_SPREAD_NODE_WORDS]; } sim_spread_node;   /* 64 bytes */

/* A sample = 8 + 8 n unsigned 64-bit words: a header, then 8 words per entry, in the order the entries were given.  All
 * words are integers and describe the state AFTER the sampled tick (what the dumps show when sim_tick == t + 1).
 *
 * Header:
 *   0   now: sim_tick after the tick (t + 1)
 *   1   running nodes
 *   2   n
 *   3   arrivals latched by this sample, over all entries
 *   4   entries with at least one arrival so far
 *   5   entries every running node has an arrival for (0 while nobody runs)
 *   6, 7   0
 * Entry i, words 8 + 8 i ..:
 *   0   id: key | (uint64_t)kind << 32
 *   1   val: ltime
 *   2   new: nodes latched by this sample
 *   3   reached: nodes with a non-zero arrival, running or not
 *   4   reached_up: running nodes with a non-zero arrival
 *   5   holds: running nodes for which the predicate holds now (exactly sim_convergence's `seen`, the ledger's word 2)
 *   6   first: the smallest non-zero arrival, 0 if none
 *   7   last: the largest arrival
 *
 * Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_SPREAD_MAX_SAMPLES, n == 0 or
 * > SIM_SPREAD_MAX, a kind outside 1-4, a subject >= n_nodes, key 0 of an EVENT / QUERY, an ltime of 2^48 or more, two equal
 * entries, a read beyond `taken` (or into a buffer that is too small), bin_width == 0, top_k == 0 or > SIM_SPREAD_TOP_MAX,
 * an unknown rank_by, an entry >= n, nodes beyond n_nodes; SIM_ESTATE on a sharded handle, between sim_step_begin and
 * sim_step_end, for a start while a map is running and for a read / stop without one; SIM_ENOMEM when the map (n * n_nodes *
 * 4 bytes), the sample buffer or a read's scratch cannot be allocated.  Bad arguments that can be judged without a map are
 * SIM_EINVAL before "no map" / "already running" is SIM_ESTATE; an entry or node out of the running map's range is judged
 * behind that.  A call that fails changes nothing. */

/* A sample is taken — and the map latched — behind tick t (the tick during which sim_tick was t) when t >= first_tick and
 * (t - first_tick) % period == 0 and fewer than `capacity` samples have been taken; one that is due with the buffer full
 * is dropped and counted, and a dropped sample latches nothing — give the buffer the room the run needs.  A first_tick that has passed already means "now" (the handle's tick).  For EVENT / QUERY entries the ring
 * plane the predicate reads gets its memory here (as in sim_track_add). */
int sim_spread_start(sim_handle*, const sim_spread_entry* e, uint32_t n, uint32_t first_tick, uint32_t period, uint32_t capacity);
/* Samples taken / dropped so far: the host knows every sampled tick in advance, so this waits for nothing.  Both are 0
 * on a handle without a map. */
int sim_spread_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken) into out[cap_words]
 * (n * (8 + 8 * entries) <= cap_words); *n_out = n. */
int sim_spread_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Frees the map and the samples. */
int sim_spread_stop(sim_handle*);

/* The reads of the map.  Each waits for the handle's stream, computes on the device from the map and the running flags the
 * handle has now, and touches neither the map nor the samples. */

/* arrival[entry][first_node .. first_node + count - 1] into out[count] (first_node + count <= n_nodes). */
int sim_spread_map(sim_handle*, uint32_t entry, uint32_t first_node, uint32_t count, uint32_t* out);
/* SIM_SPREAD_SUMMARY_WORDS (8 + 32) words per entry into out, in the entries' order:
 *   0   id                  1   val
 *   2   first               3   last
 *   4   reached             5   reached_up
 *   6   unreached_up: running nodes with arrival 0
 *   7   the sum of arrival - first over the reached nodes
 *   8 + b   reached nodes with min((arrival - first) / bin_width, 31) == b: the last bin takes everything beyond */
int sim_spread_summary(sim_handle*, uint32_t bin_width, uint64_t* out /* (8 + 32) n words */);
/* The running nodes with arrival[entry] == 0 in ascending id: the first min(cap, *total) of them into ids (null is allowed
 * with cap == 0), their number into *n_out, the number of all of them into *total. */
int sim_spread_unreached(sim_handle*, uint32_t entry, uint32_t* ids, uint32_t cap, uint32_t* n_out, uint32_t* total);
/* top[top_k]: the worst RUNNING nodes by rank_by, worst first; records beyond the number of running nodes are zero.
 * nodes: null, or room for n_nodes records — every node's record in id order, running or not. */
int sim_spread_late(sim_handle*, uint32_t top_k, uint32_t rank_by, sim_spread_node* top, sim_spread_node* nodes /* n_nodes or NULL */);
uint32_t sim_spread_version(void);

#ifdef __cplusplus
}
#endif
#endif
