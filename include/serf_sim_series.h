/*
 * serf_sim_series.h — device-resident time series: cluster gauges sampled behind a tick, without a host poll.
 *
 * An extension of include/serf_sim.h in the style of include/serf_sim_track.h: exported by the HIP library
 * (libserf_sim.so) only, with a version of its own (sim_series_version), not part of SIM_ABI_VERSION.  The CPU oracle has
 * no series: it is the checker — every word below is a pure function of the arrays the oracle dumps (SIM_ARR_ROWS /
 * SIM_ARR_QUEUE / SIM_ARR_INBOX; tests/series_model.py).
 *
 * The trackers answer "when did rumour X reach 99 %?".  A series answers "what is the cluster doing?": how deep the
 * retransmit queues are (the reference's serf.queue.Intent / Event / Query gauges, serf/base.rs:683-740, summed over the
 * running processes), how memberlist's health score is spread, how many suspicion timers run, how far the Lamport clocks
 * are apart, what the packets in flight carry (serf.messages.sent, serf/delegate.rs:337-380).  Behind every sampled tick
 * two kernels reduce the state to one sample of SIM_SERIES_WORDS integers in a buffer on the device; the host reads the
 * samples whenever it likes: sim_step(h, n) with n >> 1 stays one asynchronous call.  A series adds no protocol state:
 * digests, events, dumps and checkpoint images do not know it (sim_snapshot holds none, sim_restore leaves a running one
 * as it is), and a handle without a started series launches, allocates and synchronises nothing for it.
 *
 * Checkpoints: sim_snapshot holds no series, sim_restore leaves a running one as it is.  It keeps the first tick and
 * the period fixed when it was started, in absolute ticks: behind a restore to tick T its samples go on behind the
 * ticks t >= T with (t - first) % period == 0, in the same buffer, and what fell between is neither taken nor
 * counted as dropped.
 *
 * Out of scope: sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED) — a sample needs the sums over ALL nodes; every
 * call below returns SIM_ESTATE on such a handle (vshards > 1 on a handle that holds every node is one handle and is
 * supported); counters that would need the handlers instrumented (serf.member.*, serf.events, serf.messages.received);
 * percentiles beyond what the bins give.
 */
#ifndef SERF_SIM_SERIES_H
#define SERF_SIM_SERIES_H

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_SERIES_VERSION 1u
#define SIM_SERIES_WORDS 64u               /* one sample = 64 x uint64_t = 512 bytes */
#define SIM_SERIES_MAX_SAMPLES (1u << 20)

/* All words are integers and describe the state AFTER the sampled tick (what the dumps show when sim_tick == t + 1).
 * "Running" = flags & SIM_RF_UP: a stopped process emits no metrics, so per-node figures count running nodes only (word
 * 39 is the one exception).  "Depth" = non-empty entries of a node's queue.  Every min and every max is 0 when no node
 * runs.  "In flight" is defined on the canonical form SIM_ARR_INBOX (fanout * PG pages per node): a packet the library
 * stores once and maps to several slots counts once per slot.
 *
 *   0       sim_tick after the tick (t + 1)
 *   1       running nodes
 *   2-5     running nodes by SIM_RF_STATE 0..3
 *   6-9     queue entries by class over running nodes (meta >> 30: memberlist, intents, queries, events)
 *   10-17   running nodes by depth bin: 0, 1, 2-3, 4-7, 8-15, 16-31, 32-63, 64 (bin = 0 for depth 0, else
 *           1 + floor(log2(depth)))
 *   18      largest depth of a running node
 *   19-26   running nodes by awareness 0..7
 *   27      running suspicion timers (non-zero susp[] entries of running nodes)
 *   28      running nodes with at least one timer
 *   29, 30  sum of n_failed, of n_left over running nodes
 *   31, 32  min, max of n_known over running nodes
 *   33-38   min, max over running nodes of clock, event_clock, query_clock, in that order
 *   39      sum of overflow over ALL nodes (the model-bound counter; equals sim_cluster_stats.overflow)
 *   40      packets in flight with at least one record
 *   41-47   records in flight by sim_kind 1..7
 *   48      sum of SIM_META_LEN64 over the records in flight (16-byte units)
 *   49-63   0 */
typedef struct sim_series_sample { uint64_t w[SIM_SERIES_WORDS]; } sim_series_sample;

/* Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_SERIES_MAX_SAMPLES, a read beyond
 * `taken`; SIM_ESTATE on a sharded handle, between sim_step_begin and sim_step_end, for a start while a series is running
 * and for a read / stop without one; SIM_ENOMEM when the sample buffer cannot be allocated.  A call that fails changes
 * nothing. */

/* A sample is taken behind tick t (the tick during which sim_tick was t) when t >= first_tick, (t - first_tick) % period
 * == 0 and fewer than `capacity` samples have been taken; one that is due with the buffer full is dropped and counted.
 * A first_tick that has passed already means "now" (the handle's tick). */
int sim_series_start(sim_handle*, uint32_t first_tick, uint32_t period, uint32_t capacity);
/* Samples taken / dropped so far: the host knows every sampled tick in advance, so this waits for nothing.  Both are 0
 * on a handle without a series. */
int sim_series_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken); *n_out = n. */
int sim_series_read(sim_handle*, uint32_t first, uint32_t n, sim_series_sample* out, uint32_t* n_out);
/* Frees the buffers; the samples are gone. */
int sim_series_stop(sim_handle*);
uint32_t sim_series_version(void);

#ifdef __cplusplus
}
#endif
#endif
