/*
 * serf_sim_qboard.h — query board on the device: for a fixed set of query ids, how each query went — acks, responses, who of
 * the nodes it was meant for answered, who stayed silent, when half / 90 % / 99 % / all of them had answered — sampled behind
 * the ticks, without a host poll.
 *
 * The tenth extension of include/serf_sim.h, in the style of include/serf_sim_spread.h: exported by the HIP library
 * (libserf_sim.so) only, with a version of its own (sim_qboard_version), not part of SIM_ABI_VERSION.  The CPU oracle has no
 * board: it is the checker — every word below is a pure function of what the oracle gives behind a tick (sim_query_status,
 * sim_query_responders, the SIM_ARR_ROWS dump) and of the filter and tag operations of the script (tests/qboard_model.py).
 *
 * The spread map says a query REACHED a node.  The board says the node's ack reached the ORIGIN, which is what a caller of
 * Serf::query gets back.  sim_query_status / sim_query_responders answer that per query, each with two waits for the stream; the
 * board answers it for up to 64 queries behind every sampled tick with none.  A board adds no protocol state: digests, events,
 * dumps, checkpoint images do not know it, and a handle without a started board launches, allocates and synchronises nothing
 * for it.
 *
 * Checkpoints: sim_snapshot holds no board, sim_restore leaves a running one as it is — its records, its first tick and its
 * period, in absolute ticks (the wording of include/serf_sim_ledger.h).
 *
 * An ENTRY is a query id: non-zero, SIM_QBOARD_MAX of them at most, no two equal.  The id need not be running yet — name the
 * ids, schedule the queries, step once.  Two entries may share a residue id % SIM_QT (the running-query table is direct-mapped):
 * the later query then displaces the earlier one.  The set of entries is fixed for the board's life: stop and start to change it.
 *
 * For node l and entry e, while e's id OWNS its table entry (the entry id % SIM_QT of the running-query table names it):
 *   running    SIM_RF_UP is set
 *   admitted   the query's filters let l process it (should_process_query: the filter record and the tag classes as they are
 *              NOW; a record another query has taken over filters nothing)
 *   eligible   running and admitted
 *   open       (uint32_t)now <= deadline, as sim_query_status defines it
 *
 * Out of scope: sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED) — every call below returns SIM_ESTATE on such a handle
 * (vshards > 1 on a handle that holds every node is one handle and is supported).  Both fan-out models are supported.
 */
#ifndef SERF_SIM_QBOARD_H
#define SERF_SIM_QBOARD_H

#include <stddef.h>

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_QBOARD_VERSION 1u
#define SIM_QBOARD_MAX 64u            /* entries per board */
#define SIM_QBOARD_MAX_SAMPLES (1u << 20)
#define SIM_QBOARD_HEADER_WORDS 8u
#define SIM_QBOARD_ENTRY_WORDS 16u
#define SIM_QBOARD_TOP_MAX 64u
#define SIM_QBOARD_NODE_WORDS 8u

/* an entry's state (the high half of its word 0) */
#define SIM_QBOARD_WAITING 0u         /* the id has not owned its table entry in any sample so far */
#define SIM_QBOARD_OPEN 1u
#define SIM_QBOARD_CLOSED 2u
#define SIM_QBOARD_DISPLACED 3u       /* the id owned the entry at an earlier sample and another id owns it now */

/* what sim_qboard_top ranks the running nodes by */
#define SIM_QBOARD_BY_SILENT_ACK 0u   /* (silent_ack descending, id ascending) */
#define SIM_QBOARD_BY_SILENT_RESP 1u  /* (silent_resp descending, id ascending) */

/* One node's record over the entries that own their table entry NOW:
 *   0   id | (uint64_t)running << 32      (running: whether the node runs now)
 *   1   asked: entries that admit the node
 *   2   acked: entries whose ack bitmap has the node's bit
 *   3   responded: likewise, the response bitmap
 *   4   silent_ack: entries that admit the node, carry SIM_F_ACK and have no ack bit of it
 *   5   silent_resp: likewise for SIM_F_RESPOND and the response bit
 *   6-7 0 */
typedef struct sim_qboard_node { uint64_t w[SIM_QBOARD_NODE_WORDS]; } sim_qboard_node;   /* 64 bytes */

/* A sample = 8 + 16 n unsigned 64-bit words: a header, then 16 words per entry, in the order the ids were given.  All words
 * are integers and describe the state AFTER the sampled tick (now = t + 1: what sim_query_status says when sim_tick == t + 1).
 *
 * Header:
 *   0   now: sim_tick after the tick (t + 1)
 *   1   running nodes
 *   2   n
 *   3   entries open          4   entries closed
 *   5   entries waiting       6   entries displaced
 *   7   acks plus responses newly seen by this sample, over all entries (the sum of words 9 and 10)
 * Entry i, words 8 + 16 i ..:
 *   0   id | (uint64_t)state << 32
 *   1   origin | (uint64_t)flags << 32        (the table entry's: flags as SIM_OP_QUERY took them)
 *   2   deadline
 *   3   acks: bits set in the ack bitmap — exactly sim_query_status's figure
 *   4   responses: likewise
 *   5   eligible
 *   6   answered: eligible nodes with the ack bit
 *   7   responded: eligible nodes with the response bit
 *   8   silent = eligible - answered
 *   9   new acks since this entry's previous sample
 *   10  new responses since this entry's previous sample
 *   11-15   t_first, t_half, t_90, t_99, t_all
 *
 * The latches (words 11-15) hold the `now` of the first sample that met their condition, 0 while unset.  They are set once, and
 * set only in a sample where the entry is open and eligible > 0.  The conditions are the trackers' (include/serf_sim_track.h),
 * applied to a = answered against e = eligible:  a >= 1,  2 a >= e,  10 a >= 9 e,  100 a >= 99 e,  a == e.
 *
 * What is live in each state:
 *   waiting     words 1-15 are 0
 *   open, closed   all words
 *   displaced   words 1, 2 and 11-15 keep their last values; words 3-10 are 0
 * A query that takes its table entry over again under the SAME id (a second SIM_OP_QUERY: another deadline, origin or flags in
 * the table than at the entry's previous sample) starts the entry afresh — previous counts and latches are 0 — and is state 1;
 * so does an id that comes back behind a displacement.  A query already running at the first sample is open or closed as the
 * table says, and its `new` words are all it has.
 *
 * Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_QBOARD_MAX_SAMPLES, n == 0 or
 * > SIM_QBOARD_MAX, an id of 0, two equal ids, a read beyond `taken` (or into a buffer that is too small), `which` above 1, top_k
 * == 0 or > SIM_QBOARD_TOP_MAX, an unknown rank_by, an entry >= n, nodes beyond n_nodes; SIM_ESTATE on a sharded handle, between
 * sim_step_begin and sim_step_end, for a start while a board is running and for a read / stop without one; SIM_ENOMEM when the
 * board, the sample buffer or a read's scratch cannot be allocated.  Bad arguments that can be judged without a board are
 * SIM_EINVAL before "no board" / "already running" is SIM_ESTATE; an entry or node out of the running board's range is judged
 * behind that.  A call that fails changes nothing. */

/* A sample is taken behind tick t (the tick during which sim_tick was t) when t >= first_tick and (t - first_tick) % period == 0
 * and fewer than `capacity` samples have been taken; one that is due with the buffer full is dropped and counted, and a dropped
 * sample changes nothing — no latch, no previous count.  A first_tick that has passed already means "now" (the handle's tick). */
int sim_qboard_start(sim_handle*, const uint32_t* ids, uint32_t n, uint32_t first_tick, uint32_t period, uint32_t capacity);
/* Samples taken / dropped so far: the host knows every sampled tick in advance, so this waits for nothing.  Both are 0 on a
 * handle without a board. */
int sim_qboard_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken) into out[cap_words]
 * (n * (8 + 16 * entries) <= cap_words); *n_out = n. */
int sim_qboard_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Frees the board and the samples. */
int sim_qboard_stop(sim_handle*);
/* One stateless sample of the state the handle is in now into out[8 + 16 n], with or without a running board, for ids of its
 * own: latches and `new` words are 0, an id that does not own its entry is waiting.  The bulk form of n sim_query_status calls,
 * with one wait for the stream. */
int sim_qboard_now(sim_handle*, const uint32_t* ids, uint32_t n, uint64_t* out);

/* The reads of a running board.  Each waits for the handle's stream, computes on the device from the state the handle is in
 * now, and touches neither the board nor the samples.  They are taken over the entries that own their table entry now. */

/* The eligible nodes of `entry` without the ack bit (which 0) or the response bit (which 1) in ascending id: the first min(cap,
 * *total) of them into ids (null is allowed with cap == 0), their number into *n_out, the number of all of them into *total.
 * An entry that is waiting or displaced gives total 0. */
int sim_qboard_silent(sim_handle*, uint32_t entry, uint32_t which, uint32_t* ids, uint32_t cap, uint32_t* n_out, uint32_t* total);
/* The records of nodes first_node .. first_node + count - 1 into out[count] (first_node + count <= n_nodes). */
int sim_qboard_nodes(sim_handle*, uint32_t first_node, uint32_t count, sim_qboard_node* out);
/* top[top_k]: the worst RUNNING nodes by rank_by, worst first, ties in ascending id; records beyond the number of running nodes
 * are zero.  nodes: null, or room for n_nodes records — every node's record in id order, running or not. */
int sim_qboard_top(sim_handle*, uint32_t top_k, uint32_t rank_by, sim_qboard_node* top, sim_qboard_node* nodes /* n_nodes or NULL */);
uint32_t sim_qboard_version(void);

#ifdef __cplusplus
}
#endif
#endif
