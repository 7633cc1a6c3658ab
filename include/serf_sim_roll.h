/*
 * serf_sim_roll.h — observer roll on the device: per running node, how far its view of the subjects lags and whom it
 * accuses, binned over the cluster and ranked, sampled behind a tick, without a host poll.
 *
 * The fourth extension of include/serf_sim.h, in the style of include/serf_sim_track.h, include/serf_sim_series.h and
 * include/serf_sim_census.h: exported by the HIP library (libserf_sim.so) only, with a version of its own
 * (sim_roll_version), not part of SIM_ABI_VERSION.  The CPU oracle has no roll: it is the checker — every word below is a
 * pure function of the arrays the oracle dumps (SIM_ARR_VIEW / SIM_ARR_SLOTMAP / SIM_ARR_ROWS; tests/roll_model.py).
 *
 * The census reduces the cluster per SUBJECT: a running member is held Failed by so many observers.  It cannot say
 * whether that is every node being slightly wrong or a few nodes being badly wrong, and Lifeguard's premise is that slow
 * OBSERVERS cause the false positives.  The roll reduces the same head planes along the other axis: one record per
 * observer — how many subjects it does not know or knows at an older time than somebody else, how many running members
 * it holds Failed or Suspect, how many stopped ones it still holds Alive — a header of cluster-wide sums, maxima and a
 * histogram over the observers, and the top_k worst observers by a chosen score.  Behind every sampled tick the census's
 * count and fold kernels leave the per-subject references, then one kernel sweeps the head plane of every allocated
 * view slot once more with an observer per lane, and one folds; the host reads the samples whenever it likes:
 * sim_step(h, n) with n >> 1 stays one asynchronous call.  A roll adds no protocol state: digests, events, dumps and
 * checkpoint images do not know it (sim_snapshot holds none, sim_restore leaves a running one as it is), and a handle
 * without a started roll launches, allocates and synchronises nothing for it.
 *
 * Checkpoints: sim_snapshot holds no roll, sim_restore leaves a running one as it is.  It keeps the first tick and
 * the period fixed when it was started, in absolute ticks: behind a restore to tick T its samples go on behind the
 * ticks t >= T with (t - first) % period == 0, in the same buffer, and what fell between is neither taken nor
 * counted as dropped.
 *
 * SUBJECT: a node id that owns a view slot now (subject_of[slot] is a node).  As in the census, a subject without a slot
 * sits at its baseline, where every observer agrees by construction: it is NOT in the roll.
 * OBSERVER: every running node (flags & SIM_RF_UP) of the handle, the subject itself included.
 * PER SUBJECT a, over the observers whose entry of a's slot is known (e.bits & SIM_VB_KNOWN):
 *   ltmax_a    the max of e.ltime        (census word 13)
 *   incmax_a   the max of e.inc          (census word 15)
 *   anyknown_a whether any observer's entry is known
 *   run_a      whether the subject's own process runs (ground truth)
 * PER OBSERVER i, over all subjects a, with e = i's entry of a's slot, known = e.bits & SIM_VB_KNOWN,
 * st = SIM_VB_STATUS(e.bits), swim = SIM_VB_SWIM(e.bits):
 *   unknown      the number of a with !known && anyknown_a
 *   behind       the number of a with known && (e.ltime < ltmax_a || e.inc < incmax_a)
 *   stale        unknown + behind
 *   false_failed the number of a with run_a && known && st == SIM_STATUS_FAILED
 *   suspects     the number of a with run_a && known && swim in {SIM_SWIM_SUSPECT, SIM_SWIM_DEAD}
 *   stale_alive  the number of a with !run_a && known && st == SIM_STATUS_ALIVE
 *   lag          the sum over known entries of ltmax_a - e.ltime (64 bits)
 *
 * Out of scope: sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED) — the references need ALL observers; every call
 * below returns SIM_ESTATE on such a handle (vshards > 1 on a handle that holds every node is one handle and is
 * supported); subjects without a slot; ranking by lag.
 */
#ifndef SERF_SIM_ROLL_H
#define SERF_SIM_ROLL_H

#include <stddef.h>

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_ROLL_VERSION 1u
#define SIM_ROLL_NODE_WORDS 8u             /* an observer's record: 8 x uint64_t = 64 bytes */
#define SIM_ROLL_HEADER_WORDS 32u          /* a sample's header: 32 x uint64_t = 256 bytes */
#define SIM_ROLL_TOP_MAX 64u
#define SIM_ROLL_MAX_SAMPLES (1u << 20)

/* what the listed observers are ranked by */
#define SIM_ROLL_BY_STALE 0u               /* stale */
#define SIM_ROLL_BY_ACCUSED 1u             /* false_failed + suspects */
#define SIM_ROLL_BY_MISSED 2u              /* stale_alive */

/* All words are integers and describe the state AFTER the sampled tick (what the dumps show when sim_tick == t + 1).
 *
 * One node:
 *   0   id | (uint64_t)running << 32
 *   1   stale            2   unknown          3   false_failed     4   suspects
 *   5   stale_alive      6   lag              7   behind
 * A node that does not run observes nothing: words 1-7 are 0. */
typedef struct sim_roll_node { uint64_t w[SIM_ROLL_NODE_WORDS]; } sim_roll_node;

/* One sample's header.  Sums, maxima and counts are over the observers (the running nodes).
 *   0       sim_tick after the tick (t + 1)
 *   1       running nodes
 *   2       subjects (allocated slots)
 *   3       listed | (uint64_t)rank_by << 32
 *   4       observers with stale == 0
 *   5       the sum of stale                      6   the max of stale
 *   7       the sum of unknown
 *   8       observers with false_failed > 0       9   the sum of false_failed
 *   10      observers with suspects > 0          11   the sum of suspects
 *   12      observers with stale_alive > 0       13   the sum of stale_alive
 *   14      the sum of lag                       15   the max of lag
 *   16-31   observers by stale bin: bin 0 holds stale == 0, otherwise the bin is 1 + floor(log2(stale)), capped at 15
 *           (0, 1, 2-3, 4-7, ...)
 * With no running node everything except words 0, 2 and the rank_by half of word 3 is 0.  Words 9, 11 and 13 equal the
 * census header's words 6, 8 and 10 of the same state, by construction. */
typedef struct sim_roll_header { uint64_t w[SIM_ROLL_HEADER_WORDS]; } sim_roll_header;

/* A sample = one header, then `top_k` node records: the worst observers by the score `rank_by` names, in descending
 * score, ties in ascending node id.  Observers with score 0 are never listed; `listed` records are stored, the rest stay
 * zero.  The stride (32 + 8 * top_k) words is fixed: a range of samples is one copy.
 *
 * Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_ROLL_MAX_SAMPLES, top_k == 0 or
 * > SIM_ROLL_TOP_MAX, an unknown rank_by, a read beyond `taken` (or into a buffer that is too small); SIM_ESTATE on a
 * sharded handle, between sim_step_begin and sim_step_end, for a start while a roll is running and for a read / stop
 * without one; SIM_ENOMEM when the buffers cannot be allocated.  A call that fails changes nothing. */

/* A sample is taken behind tick t (the tick during which sim_tick was t) when t >= first_tick, (t - first_tick) % period
 * == 0 and fewer than `capacity` samples have been taken; one that is due with the buffer full is dropped and counted.
 * A first_tick that has passed already means "now" (the handle's tick). */
int sim_roll_start(sim_handle*, uint32_t first_tick, uint32_t period, uint32_t capacity, uint32_t top_k, uint32_t rank_by);
/* Samples taken / dropped so far: the host knows every sampled tick in advance, so this waits for nothing.  Both are 0
 * on a handle without a roll. */
int sim_roll_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken) into out[cap_words]
 * (n * (32 + 8 * top_k) <= cap_words); *n_out = n. */
int sim_roll_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Frees the buffers; the samples are gone. */
int sim_roll_stop(sim_handle*);
/* The bulk counterpart of sim_members: the same kernels, once, on the state the handle is in now — with or without a
 * running roll, which it does not touch — and a wait for the stream.  Fills *hdr and top[top_k] (records beyond `listed`
 * zero); `nodes` is null, or room for n_nodes records: every node's record in id order, a stopped node's all zero but
 * the id. */
int sim_roll_now(sim_handle*, uint32_t top_k, uint32_t rank_by, sim_roll_header* hdr, sim_roll_node* top, sim_roll_node* nodes);
uint32_t sim_roll_version(void);

#ifdef __cplusplus
}
#endif
#endif
