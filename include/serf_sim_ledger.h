/*
 * serf_sim_ledger.h — rumour ledger on the device: for a fixed set of record identities, how many running nodes have applied
 * the rumour, how many copies of it wait in the retransmit queues and how many travel in packets, sampled behind a tick,
 * without a host poll.
 *
 * The fifth extension of include/serf_sim.h, in the style of include/serf_sim_track.h, include/serf_sim_series.h,
 * include/serf_sim_census.h and include/serf_sim_roll.h: exported by the HIP library (libserf_sim.so) only, with a version
 * of its own (sim_ledger_version), not part of SIM_ABI_VERSION.  The CPU oracle has no ledger: it is the checker — every
 * word below is a pure function of the arrays the oracle dumps (SIM_ARR_ROWS / SIM_ARR_QUEUE / SIM_ARR_INBOX) and of
 * sim_convergence_many (tests/ledger_model.py).
 *
 * The trackers, the series, the census and the roll say who knows what and who is behind.  The ledger says what a rumour
 * COSTS and when it DIES: the curve of its spread tick by tick, the copies the cluster sends for it (the price of
 * retransmit_mult, fanout and the packet budget), the tick at which the last copy leaves the last queue — and whether
 * that happened before everybody had it.  With period 1 the sum of an entry's word 6 over the samples is the number of
 * copies the cluster sent.  A ledger adds no protocol state: digests, events, dumps, checkpoint images do not know it, and
 * a handle without a started ledger launches, allocates and synchronises nothing for it.
 *
 * Checkpoints: sim_snapshot holds no ledger, sim_restore leaves a running one as it is.  It keeps the first tick and
 * the period fixed when it was started, in absolute ticks: behind a restore to tick T its samples go on behind the
 * ticks t >= T with (t - first) % period == 0, in the same buffer, and what fell between is neither taken nor
 * counted as dropped.
 *
 * An ENTRY names a record identity:
 *   kind   SIM_K_JOIN .. SIM_K_DEAD (1-7)
 *   key    JOIN / LEAVE / ALIVE / SUSPECT / DEAD: the subject (< n_nodes); EVENT / QUERY: the event key or query id, non-zero
 *   val    kinds 1-4: the Lamport time, below 2^48; ALIVE: the incarnation; SUSPECT / DEAD: the incarnation, below 2^24 —
 *          the accuser is not part of the identity
 * Flags, length, class, transmits and queue id are not part of the identity either.
 * A queued record (sim_record as SIM_ARR_QUEUE shows it) MATCHES an entry when kind and key are equal and val is equal —
 * for SUSPECT / DEAD (rec.val & 0xFFFFFF) == val.  A record on the wire (sim_packet) matches likewise on its 48 value
 * bits — for SUSPECT / DEAD their low 24.  The set of entries is fixed for the ledger's life: stop and start to change it.
 *
 * "Running" and "in flight" are those of include/serf_sim_series.h: queues are counted over running nodes only, packets on
 * the canonical form SIM_ARR_INBOX — a packet stored once and mapped to several fan-out slots counts once per slot,
 * whether or not its receiver runs.
 *
 * Out of scope: sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED) — every call below returns SIM_ESTATE on such a
 * handle (vshards > 1 on a handle that holds every node is one handle and is supported); the reach of ALIVE / SUSPECT /
 * DEAD (follow those with a SIM_TRK_MEMBER tracker).
 */
#ifndef SERF_SIM_LEDGER_H
#define SERF_SIM_LEDGER_H

#include <stddef.h>

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_LEDGER_VERSION 1u
#define SIM_LEDGER_MAX 64u            /* entries per ledger (= SIM_CONV_MAX) */
#define SIM_LEDGER_MAX_SAMPLES (1u << 20)
#define SIM_LEDGER_HEADER_WORDS 8u
#define SIM_LEDGER_ENTRY_WORDS 8u

typedef struct sim_ledger_entry { uint32_t kind; uint32_t key; uint64_t val; } sim_ledger_entry;   /* 16 bytes */

/* A sample = 8 + 8 n unsigned 64-bit words: a header, then 8 words per entry, in the order the entries were given.  All
 * words are integers and describe the state AFTER the sampled tick (what the dumps show when sim_tick == t + 1).
 *
 * Header:
 *   0   sim_tick after the tick (t + 1)
 *   1   running nodes
 *   2   n
 *   3   queued records of running nodes, all identities (= series words 6 + 7 + 8 + 9)
 *   4   records in flight, all identities (= series words 41 .. 47 summed)
 *   5   packets in flight with at least one record (= series word 40)
 *   6   the sum of SIM_META_TRANSMITS over the records of word 3
 *   7   0
 * Entry i, words 8 + 8 i ..:
 *   0   key | (uint64_t)kind << 32
 *   1   val
 *   2   reach: running nodes for which SIM_TRK_RUMOUR's predicate holds (kinds 1-4, exactly sim_convergence); 0 for kinds 5-7
 *   3   holders: running nodes whose queue holds at least one matching record
 *   4   queued: matching records in the queues of running nodes (can exceed holders)
 *   5   transmits: the sum of SIM_META_TRANSMITS over them
 *   6   in flight: matching records in the packets in flight
 *   7   fresh: those of word 4 with transmits 0 (learnt, not yet sent: the wavefront)
 *
 * Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_LEDGER_MAX_SAMPLES, n == 0 or
 * > SIM_LEDGER_MAX, a kind outside 1-7, a subject >= n_nodes, key 0 of an EVENT / QUERY, a val beyond the bounds above, two
 * equal entries, a read beyond `taken` (or into a buffer that is too small); SIM_ESTATE on a sharded handle, between
 * sim_step_begin and sim_step_end, for a start while a ledger is running and for a read / stop without one; SIM_ENOMEM
 * when the buffers cannot be allocated.  A call that fails changes nothing. */

/* A sample is taken behind tick t (the tick during which sim_tick was t) when t >= first_tick, (t - first_tick) % period
 * == 0 and fewer than `capacity` samples have been taken; one that is due with the buffer full is dropped and counted.
 * A first_tick that has passed already means "now" (the handle's tick).  For EVENT / QUERY entries the ring plane the
 * reach predicate reads gets its memory here (as in sim_track_add). */
int sim_ledger_start(sim_handle*, const sim_ledger_entry* e, uint32_t n, uint32_t first_tick, uint32_t period, uint32_t capacity);
/* Samples taken / dropped so far: the host knows every sampled tick in advance, so this waits for nothing.  Both are 0
 * on a handle without a ledger. */
int sim_ledger_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken) into out[cap_words]
 * (n * (8 + 8 * entries) <= cap_words); *n_out = n. */
int sim_ledger_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Frees the buffers; the samples are gone. */
int sim_ledger_stop(sim_handle*);
/* The same kernels, once, on the state the handle is in now — with or without a running ledger, which it does not touch,
 * and with entries of its own — and a wait for the stream.  Fills out[8 + 8 n]. */
int sim_ledger_now(sim_handle*, const sim_ledger_entry* e, uint32_t n, uint64_t* out /* 8 + 8 n words */);
uint32_t sim_ledger_version(void);

#ifdef __cplusplus
}
#endif
#endif
