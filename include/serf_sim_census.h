/*
 * serf_sim_census.h — membership census on the device: per subject, how the running nodes' views of it agree, sampled
 * behind a tick, without a host poll.
 *
 * The third extension of include/serf_sim.h, in the style of include/serf_sim_track.h and include/serf_sim_series.h:
 * exported by the HIP library (libserf_sim.so) only, with a version of its own (sim_census_version), not part of
 * SIM_ABI_VERSION.  The CPU oracle has no census: it is the checker — every word below is a pure function of the arrays
 * the oracle dumps (SIM_ARR_VIEW / SIM_ARR_SLOTMAP / SIM_ARR_ROWS; tests/census_model.py).
 *
 * The trackers answer "when did verdict Y about subject X reach 99 %?" for subjects named in advance; a series answers
 * "what is the cluster doing?".  A census answers what serf is about: do the membership views agree, and where they do
 * not, about whom and how badly — running nodes that others hold Suspect or Failed (the false positives of the SWIM and
 * Lifeguard papers, which hit subjects nobody can name beforehand), stopped nodes somebody still holds Alive, the time
 * until every affected member's entry is the same everywhere.  Behind every sampled tick three kernels stream the head
 * plane of every allocated view slot once (16 bytes per (slot, node)) and reduce it to one record per subject plus a
 * header of cluster-wide figures, in a buffer on the device; the host reads the samples whenever it likes: sim_step(h, n)
 * with n >> 1 stays one asynchronous call.  A census adds no protocol state: digests, events, dumps and checkpoint
 * images do not know it (sim_snapshot holds none, sim_restore leaves a running one as it is), and a handle without a
 * started census launches, allocates and synchronises nothing for it.
 *
 * Checkpoints: sim_snapshot holds no census, sim_restore leaves a running one as it is.  It keeps the first tick and
 * the period fixed when it was started, in absolute ticks: behind a restore to tick T its samples go on behind the
 * ticks t >= T with (t - first) % period == 0, in the same buffer, and what fell between is neither taken nor
 * counted as dropped.
 *
 * SUBJECT: a node id that owns a view slot now (subject_of[slot] is a node).  A subject without a slot sits at its
 * baseline, where every observer agrees by construction: it is NOT in the census.  On a dense handle (view_slots == 0
 * or >= n_nodes) every node owns slot == id: the census covers all N subjects and a sample costs N * N entries —
 * QUADRATIC in the cluster's size; dense handles are small clusters.
 * OBSERVER: every running node (flags & SIM_RF_UP) of the handle, the subject itself included.
 * For an observer's entry e of the subject's slot: known = e.bits & SIM_VB_KNOWN, st = known ? SIM_VB_STATUS(e.bits) :
 * SIM_STATUS_NONE.
 *
 * Out of scope: sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED) — a census needs the sums over ALL observers;
 * every call below returns SIM_ESTATE on such a handle (vshards > 1 on a handle that holds every node is one handle and
 * is supported); subjects without a slot; per-observer output (sim_members is that for one observer; the observer roll,
 * include/serf_sim_roll.h, reduces the same planes per observer).
 */
#ifndef SERF_SIM_CENSUS_H
#define SERF_SIM_CENSUS_H

#include <stddef.h>

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_CENSUS_VERSION 1u
#define SIM_CENSUS_WORDS 16u               /* a subject's record and a sample's header: 16 x uint64_t = 128 bytes each */
#define SIM_CENSUS_MAX_SAMPLES (1u << 20)

/* All words are integers and describe the state AFTER the sampled tick (what the dumps show when sim_tick == t + 1).
 *
 * One subject:
 *   0       subject | (uint64_t)slot << 32
 *   1       bit 0: the subject's own process is running (ground truth)
 *   2-6     observers by st = NONE, ALIVE, LEAVING, LEFT, FAILED (they sum to the running nodes)
 *   7-10    known observers by SIM_VB_SWIM 0..3 (they sum to the running nodes - word 2)
 *   11      observers with !known && SIM_VB_INTENT(e.bits) != 0 (a buffered intent)
 *   12, 13  min, max of e.ltime over the known observers (0, 0 when there is none)
 *   14, 15  min, max of e.inc over the known observers (0, 0 when there is none) */
typedef struct sim_census_subject { uint64_t w[SIM_CENSUS_WORDS]; } sim_census_subject;

/* One sample's header.  A subject is SETTLED when one st bin holds every observer and, if that bin is not NONE, one swim
 * bin holds them all, word 12 == word 13 and word 14 == word 15.  Words 4-11 cover ALL subjects, also those whose records
 * `max_subjects` cut off.  With no running node they are all 0 (nobody observes: no subject is settled).
 *   0       sim_tick after the tick (t + 1)
 *   1       running nodes
 *   2       subjects (allocated slots)
 *   3       records stored = min(word 2, max_subjects)
 *   4       settled subjects
 *   5       running subjects with FAILED (word 6) > 0                         6   the sum of that count over them
 *   7       running subjects with swim SUSPECT + DEAD (words 8, 9) > 0         8   the sum of that count over them
 *   9       stopped subjects with ALIVE (word 3) > 0                          10   the sum of that count over them
 *   11      stopped subjects with FAILED + LEFT == running nodes (everybody knows)
 *   12-15   0 */
typedef struct sim_census_header { uint64_t w[SIM_CENSUS_WORDS]; } sim_census_header;

/* A sample = one header, then `max_subjects` records: the subjects in ascending SLOT order, the first max_subjects of
 * them; records beyond word 3 are zero.  The stride (1 + max_subjects) * SIM_CENSUS_WORDS words is fixed: a range of
 * samples is one copy.
 *
 * Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_CENSUS_MAX_SAMPLES, max_subjects
 * == 0, a read beyond `taken` (or into a buffer that is too small); SIM_ESTATE on a sharded handle, between
 * sim_step_begin and sim_step_end, for a start while a census is running and for a read / stop without one; SIM_ENOMEM
 * when the buffers cannot be allocated.  A call that fails changes nothing. */

/* A sample is taken behind tick t (the tick during which sim_tick was t) when t >= first_tick, (t - first_tick) % period
 * == 0 and fewer than `capacity` samples have been taken; one that is due with the buffer full is dropped and counted.
 * A first_tick that has passed already means "now" (the handle's tick). */
int sim_census_start(sim_handle*, uint32_t first_tick, uint32_t period, uint32_t capacity, uint32_t max_subjects);
/* Samples taken / dropped so far: the host knows every sampled tick in advance, so this waits for nothing.  Both are 0
 * on a handle without a census. */
int sim_census_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken) into out[cap_words]
 * (n * (1 + max_subjects) * SIM_CENSUS_WORDS <= cap_words); *n_out = n. */
int sim_census_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Frees the buffers; the samples are gone. */
int sim_census_stop(sim_handle*);
/* The bulk counterpart of sim_members: the same kernels, once, on the state the handle is in now — with or without a
 * running census, which it does not touch — and a wait for the stream.  Fills *hdr (word 3 = *n) and the first
 * *n = min(subjects, cap) records of recs[cap]; recs may be null when cap == 0. */
int sim_census_now(sim_handle*, sim_census_header* hdr, sim_census_subject* recs, uint32_t cap, uint32_t* n);
uint32_t sim_census_version(void);

#ifdef __cplusplus
}
#endif
#endif
