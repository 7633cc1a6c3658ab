/*
 * serf_sim_track.h — device-resident trackers: dissemination and failure-detection latency without a host poll.
 *
 * An extension of include/serf_sim.h, exported by the HIP library (libserf_sim.so) only; it has a version of its own
 * (sim_track_version) and is not part of SIM_ABI_VERSION.  The CPU oracle has no trackers: it is the checker — every
 * figure below is computable from the oracle stepped one tick at a time (tests/track_model.py).
 *
 * The host registers what it wants followed.  Behind every tick the library counts, on the GPU, how many RUNNING nodes
 * satisfy each tracker's predicate, latches the tick at which each threshold was first crossed and retires the tracker.
 * The host reads a few bytes per tracker whenever it likes: sim_step(h, n) with n >> 1 stays one asynchronous call.
 * Trackers add no protocol state: digests, events, dumps and checkpoint images do not know them, and a handle without
 * a registered tracker launches, allocates and synchronises nothing for them.
 *
 * Out of scope:
 *   - sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED): a latch needs the count over ALL nodes; per-shard counts
 *     would have to travel beside the round's exchange.  Every call below returns SIM_ESTATE on such a handle.
 *     (vshards > 1 on a handle that holds every node is one handle and is supported.)
 *   - the count of every tick as a curve: only the latches, the peak and the last count are kept;
 *   - resolving a user event's / query's Lamport time on the device: the host passes it, as for sim_convergence
 *     (sim_stats_get(node).event_time / query_time BEFORE the call that originates it);
 *   - checkpoints: sim_snapshot does not hold trackers, sim_restore leaves the registered ones as they are.  A window
 *     keeps the absolute ticks fixed at registration: a tracker whose window lies before the restored tick is never
 *     evaluated and stays in state 0 until it is removed; one whose window straddles it is evaluated from the restored
 *     tick to the window's end.
 */
#ifndef SERF_SIM_TRACK_H
#define SERF_SIM_TRACK_H

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_TRACK_VERSION 1u
#define SIM_TRACK_MAX 1024u            /* trackers registered on one handle at a time */
#define SIM_TRACK_NEVER 0xFFFFFFFFu

enum sim_track_kind { SIM_TRK_RUMOUR = 1, SIM_TRK_MEMBER = 2 };

/* The entry e of (node, subject) below is the node's view slot of the subject, or the subject's baseline when it has
 * no view slot (what sim_members and sim_convergence read); known = e.bits & SIM_VB_KNOWN.
 *
 * SIM_TRK_RUMOUR — exactly sim_convergence's predicate:
 *   a = SIM_K_JOIN / SIM_K_LEAVE: b = subject;  hit = known && e.ltime >= ltime
 *   a = SIM_K_EVENT / SIM_K_QUERY: b = key (event key / query id, non-zero);  hit = the key is in the bucket of
 *       Lamport time `ltime` of the node's ring (its own keys or its overflow rows)
 * SIM_TRK_MEMBER — a = subject, b = status_mask | swim_mask << 8 (bit i of status_mask: enum sim_member_status i,
 *   bit j of swim_mask: enum sim_swim_state j; at least one bit set, none beyond):
 *   st = known ? SIM_VB_STATUS(e.bits) : SIM_STATUS_NONE
 *   hit = (((status_mask >> st) & 1) || (known && ((swim_mask >> SIM_VB_SWIM(e.bits)) & 1))) && e.inc >= min_inc
 *   e.g. "suspected or worse": status_mask 1 << FAILED, swim_mask 1 << SUSPECT | 1 << DEAD;  "declared failed":
 *   status_mask 1 << FAILED;  "re-join seen": status_mask 1 << ALIVE, min_inc = k. */
typedef struct sim_tracker {           /* 32 bytes */
  uint32_t kind;
  uint32_t a;          /* RUMOUR: SIM_K_JOIN / LEAVE / EVENT / QUERY      MEMBER: subject node id              */
  uint32_t b;          /* RUMOUR: key (node id, event key, query id)      MEMBER: status_mask | swim_mask << 8 */
  uint32_t min_inc;    /* MEMBER: entry's incarnation must be >= this; RUMOUR: 0                                */
  uint64_t ltime;      /* RUMOUR: Lamport time, as for sim_convergence; MEMBER: 0                               */
  uint32_t start_tick; /* first tick whose END is evaluated; one that has passed already means "now": it is
                        * replaced by the handle's tick at sim_track_add, and the window counts from there       */
  uint32_t max_age;    /* evaluated for ticks start_tick .. start_tick + max_age - 1; 0 = until `all` or removal */
} sim_tracker;

/* Evaluation happens after every tick t (the tick during which sim_tick was t) inside the window.  up = nodes with
 * SIM_RF_UP at that moment, count = those of them whose predicate holds.  A latch holds the value of sim_tick AFTER the
 * tick that crossed its threshold (t + 1), is set once and never taken back; each needs up > 0:
 *   first: count >= 1   half: 2 count >= up   p90: 10 count >= 9 up   p99: 100 count >= 99 up   all: count == up
 * A tracker retires when `all` latches or when the last tick of its window has been evaluated. */
typedef struct sim_track_result {      /* 56 bytes */
  uint32_t first, half, p90, p99, all; /* SIM_TRACK_NEVER until latched                                         */
  uint32_t evaluated;                  /* ticks evaluated so far                                                */
  uint64_t peak, last, last_up;        /* largest count seen; count and running nodes at the last evaluation    */
  uint32_t state;                      /* 0 waiting for start_tick, 1 active, 2 retired (all / age)             */
  uint32_t pad;
} sim_track_result;

/* Errors of all calls: SIM_EINVAL for null pointers, n == 0, unknown kinds, node ids >= n_nodes, a zero key, mask bits
 * that name no state (or no bit at all), fields that must be 0 and are not, ids that are not registered (or named twice
 * in one sim_track_remove); SIM_ESTATE on a sharded handle and between sim_step_begin and sim_step_end.  A call that fails changes
 * nothing. */

/* Registers n trackers; ids_out[i] (< SIM_TRACK_MAX) names tracker i until it is removed — an id is stable, a removed
 * one is handed out again (lowest first).  SIM_ERANGE when more than SIM_TRACK_MAX would be registered.  The ring
 * plane an EVENT / QUERY tracker reads gets its memory here if it had none. */
int sim_track_add(sim_handle*, const sim_tracker* t, uint32_t n, uint32_t* ids_out);
/* Frees the entries (retired trackers stay registered, and readable, until they are removed). */
int sim_track_remove(sim_handle*, const uint32_t* ids, uint32_t n);
/* Waits for the handle's stream, then copies the results of the named trackers. */
int sim_track_read(sim_handle*, const uint32_t* ids, uint32_t n, sim_track_result* out);
/* registered: entries held; active: those of them that have not retired (waits for the stream as well). */
int sim_track_active(sim_handle*, uint32_t* registered, uint32_t* active);
uint32_t sim_track_version(void);

#ifdef __cplusplus
}
#endif
#endif
