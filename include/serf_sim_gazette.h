/*
 * serf_sim_gazette.h — member gazette on the device: the member events (Join / Leave / Failed / Reap) every node's
 * application is handed, and how often a member flaps in a node's eyes, counted per node and per subject behind the
 * sampled ticks, without a host poll and without instrumenting the handlers.
 *
 * The twelfth extension of include/serf_sim.h, in the style of include/serf_sim_roll.h: exported by the HIP library
 * (libserf_sim.so) only, with a version of its own (sim_gazette_version), not part of SIM_ABI_VERSION.  The CPU oracle
 * has no gazette: it is the checker — every word below is a pure function of the arrays the oracle dumps
 * (SIM_ARR_VIEW / SIM_ARR_SLOTMAP / SIM_ARR_ROWS) at the sampled ticks (tests/gazette_model.py).
 *
 * Census, roll, detection log and series say where the cluster STANDS.  The gazette says what HAPPENS at a node: the
 * reference's rate metrics serf.member.join, serf.member.leave, serf.member.flap (serf/base.rs:1242, 1324, 1418) and the
 * member events of event.rs:325-378.  sim_watch on every node plus sim_drain_events gives the same through a bounded
 * device log that loses events at any interesting size and forces a host drain between ticks.  A member event IS a
 * change of an (observer, subject) view entry's `bits` word: the gazette keeps the previous sample's `bits` (the SHADOW)
 * and diffs them against what the tick has stored anyway.  The host reads nothing back per sample: sim_step(h, n) with n >> 1 stays
 * one asynchronous call, EXCEPT behind a tick in which the slots' high-water mark crosses a group of the shadow — then the host waits
 * for the stream, allocates the group and replaces its per-slot scratch (at most 64 times in a handle's life); an allocation that
 * fails there makes sim_step / sim_step_end return SIM_ENOMEM, the sample is not taken and a later tick tries again.  A
 * gazette adds no protocol state: digests, events, dumps and checkpoint images do not know it, and a handle without a
 * started gazette launches, allocates and synchronises nothing for it.
 *
 * DEFINITION.  sim_gazette_start takes the shadow at once: one uint32_t per (slot below the host's high-water mark, node),
 * equal to the head's `bits`, and shadow_subject[slot] = the subject that owns the slot.  (The shadow is allocated in
 * groups of slots as the high-water mark rises, never view_slots x n_nodes up front.)  Behind every sampled tick t, for
 * every allocated slot a with subject x = subject_of[a] and every node l:
 *   cur   the head `bits` of view[a][l]
 *   prev  shadow[a][l] if shadow_subject[a] == x.  Otherwise the slot is FRESH — handed out, or handed to another
 *         subject, since the last sample — and prev is the `bits` of the subject's baseline entry, which is what the
 *         column was filled with when the slot was handed out
 *   then shadow[a][l] = cur and shadow_subject[a] = x (a slot that is free now only has its shadow_subject cleared)
 *   the transition prev -> cur is COUNTED only if node l runs: a stopped process emits nothing, and recycling rewrites
 *   its column silently.
 * s(bits) = 0 when !(bits & SIM_VB_KNOWN), else SIM_VB_STATUS(bits) (1 Alive .. 4 Failed).  The swim index is
 * SIM_VB_SWIM(bits), looked at only where both sides are known.
 *
 * The eight columns of both maps:
 *   0 join       s(prev) == 0 && s(cur) != 0, or s(prev) in {Left, Failed} && s(cur) == Alive (what SIM_EV_JOIN announces)
 *   1 leave      s(cur) == Left && s(prev) not in {0, Left}
 *   2 failed     s(cur) == Failed && s(prev) not in {0, Failed}
 *   3 reap       s(prev) != 0 && s(cur) == 0
 *   4 flap       a join with s(prev) == Failed and ((t - SIM_VB_STAMP(prev)) & 0x1FFFFF) < flap_window: leave_time.elapsed()
 *                < flap_timeout of base.rs:1237-1247.  A Failed entry's stamp is its leave time, and the join zeroes it:
 *                hence the SHADOW's stamp
 *   5 suspected  swim Alive -> Suspect
 *   6 cleared    swim Suspect -> Alive
 *   7 peak       not a sum.  Node map: the most events of columns 0-3 the node had in one sample.  Subject map: the most
 *                observers that announced the subject `failed` in one sample.
 * NODE MAP    uint32_t[n_nodes][8], accumulated while the gazette runs: row l is what node l's application saw.
 * SUBJECT MAP uint32_t[n_nodes][8], keyed by subject id (not by slot): row x is how many observers announced x joined,
 *             failed, and so on.
 *
 * A SAMPLE is 64 x uint64_t:
 *   0      sim_tick after the tick (t + 1)
 *   1      running nodes
 *   2      slots looked at (allocated slots)
 *   3      fresh slots among them
 *   4-28   the 5 x 5 matrix [s(prev)][s(cur)] of this sample's counted transitions; the diagonal is 0
 *   29-44  the 4 x 4 swim matrix [swim(prev)][swim(cur)] (both sides known); the diagonal is 0
 *   45-51  the sums of columns 0-6 in this sample
 *   52     nodes with at least one event of columns 0-3
 *   53,54  the largest such count at one node, and the lowest node id that has it (0, 0 when there is none)
 *   55     subjects with at least one event of columns 0-3
 *   56,57  the subject the most observers announced `failed` (the lowest id on a tie), and by how many (0, 0: none)
 *   58-62  dead time (t - the shadow's stamp, modulo 2^21) of this sample's Failed -> Alive joins, in bins
 *          < 2, < 8, < 32, < 128, >= 128 ticks
 *   63     0
 *
 * FULL BUFFER.  A sample that is due with the buffer full is dropped and counted, and it is not looked at either: the
 * shadow and both maps stand as the last stored sample left them, so the maps are always the sums of the samples read.
 *
 * CHECKPOINTS.  sim_snapshot holds no gazette, sim_restore leaves a running one as it is, with its first tick and period
 * in absolute ticks (include/serf_sim_roll.h).  A sample that does not follow its predecessor (or the start) by exactly
 * one period — the first one behind a restore to another tick, the rumour tree's stamp rule — re-takes the whole shadow
 * and counts nothing: its word 3 equals its word 2 and every word from 4 on is 0.
 *
 * Out of scope: sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED): every call below returns SIM_ESTATE on one
 * (vshards > 1 on a handle that holds every node is one handle and is supported); serf.member.update, serf.events,
 * serf.queries and serf.messages.received.  Two events of one (observer, subject) pair between two samples show as their
 * net transition, or as none: period 1 sees every event the oracle's log has for entries that change once a tick.
 * Leaving -> Alive through a join intent is visible in the matrix only (the reference emits no event for it either).
 * The counters are 32 bits and wrap.
 */
#ifndef SERF_SIM_GAZETTE_H
#define SERF_SIM_GAZETTE_H

#include <stddef.h>

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_GAZETTE_VERSION 1u
#define SIM_GAZETTE_WORDS 64u              /* a sample: 64 x uint64_t = 512 bytes */
#define SIM_GAZETTE_COLS 8u                /* a map row: 8 x uint32_t = 32 bytes */
#define SIM_GAZETTE_TOP_MAX 64u
#define SIM_GAZETTE_MAX_SAMPLES (1u << 20)

/* the maps */
#define SIM_GAZETTE_MAP_NODES 0u
#define SIM_GAZETTE_MAP_SUBJECTS 1u
/* the columns */
#define SIM_GAZETTE_JOIN 0u
#define SIM_GAZETTE_LEAVE 1u
#define SIM_GAZETTE_FAILED 2u
#define SIM_GAZETTE_REAP 3u
#define SIM_GAZETTE_FLAP 4u
#define SIM_GAZETTE_SUSPECTED 5u
#define SIM_GAZETTE_CLEARED 6u
#define SIM_GAZETTE_PEAK 7u

typedef struct sim_gazette_sample { uint64_t w[SIM_GAZETTE_WORDS]; } sim_gazette_sample;
typedef struct sim_gazette_row { uint32_t c[SIM_GAZETTE_COLS]; } sim_gazette_row;
/* a place of a ranking: the row's id (0xFFFFFFFF, and a row of zeros, for a place beyond n_nodes) and the row */
typedef struct sim_gazette_rank { uint64_t id; sim_gazette_row row; } sim_gazette_rank;

/* Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_GAZETTE_MAX_SAMPLES, flap_window
 * >= SIM_INTERVAL_LIMIT, an unknown map or column, k == 0 or > SIM_GAZETTE_TOP_MAX, a read beyond `taken` or beyond
 * n_nodes (or into a buffer that is too small); SIM_ESTATE on a sharded handle, between sim_step_begin and sim_step_end,
 * for a start while a gazette is running and for a read / stop without one; SIM_ENOMEM when the buffers cannot be
 * allocated.  A call that fails changes nothing. */

/* Takes the shadow of the state the handle is in and zeroes both maps.  A sample is taken behind tick t (the tick during
 * which sim_tick was t) when t >= first_tick, (t - first_tick) % period == 0 and fewer than `capacity` samples have been
 * taken.  A first_tick that has passed already means "now" (the handle's tick). */
int sim_gazette_start(sim_handle*, uint32_t first_tick, uint32_t period, uint32_t capacity, uint32_t flap_window);
/* Samples taken / dropped so far; waits for nothing.  Both are 0 on a handle without a gazette. */
int sim_gazette_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken) into out[cap_words]
 * (n * 64 <= cap_words); *n_out = n. */
int sim_gazette_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Rows first .. first + n - 1 (first + n <= n_nodes) of the node map / the subject map as they stand behind the samples
 * enqueued so far; waits for the handle's stream. */
int sim_gazette_nodes(sim_handle*, uint32_t first, uint32_t n, sim_gazette_row* out);
int sim_gazette_subjects(sim_handle*, uint32_t first, uint32_t n, sim_gazette_row* out);
/* ALL rows of `map` ranked on the device by `column`, descending, ties in ascending id: the first k into out[k]. */
int sim_gazette_top(sim_handle*, uint32_t map, uint32_t column, uint32_t k, sim_gazette_rank* out);
/* Frees the samples, the maps and the shadow. */
int sim_gazette_stop(sim_handle*);
uint32_t sim_gazette_version(void);

#ifdef __cplusplus
}
#endif
#endif
