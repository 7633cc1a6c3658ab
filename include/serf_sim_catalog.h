/*
 * serf_sim_catalog.h — rumour catalogue on the device: the record identities that are LIVE in the cluster, found behind a tick,
 * not named in advance — and a registry of every identity that was ever found, with when it was first and last seen, its peaks
 * and the copies it cost.
 *
 * An extension of include/serf_sim.h in the style of include/serf_sim_ledger.h: exported by the HIP library (libserf_sim.so)
 * only, with a version of its own (sim_catalog_version), not part of SIM_ABI_VERSION.  The CPU oracle has no catalogue: it is
 * the checker — every word below is a pure function of the arrays the oracle dumps (SIM_ARR_ROWS / SIM_ARR_QUEUE /
 * SIM_ARR_INBOX) behind the sampled ticks (tests/catalog_model.py).
 *
 * The ledger, the spread map and the rumour tree follow identities somebody names.  That works for what the host injects.  The
 * SUSPECT, DEAD and refuting ALIVE records of a cluster under churn and loss, the intents a rejoin or a reap produces, what
 * sim_deliver_message and SIM_OP_RECONNECT bring in — the protocol makes those itself, with incarnations and Lamport times
 * nobody outside knows.  The catalogue lists them; feed what it finds to the ledger, the spread map or the tree.  A catalogue
 * adds no protocol state: digests, events, dumps, checkpoint images do not know it, and a handle without a started catalogue
 * launches, allocates and synchronises nothing for it.
 *
 * Checkpoints: sim_snapshot holds no catalogue, sim_restore leaves a running one as it is (as the ledger: first tick and
 * period stay, in absolute ticks; the registry and the previous sample's set stay as well).
 *
 * IDENTITY (that of include/serf_sim_ledger.h): id = key | (uint64_t)kind << 32 for the kinds SIM_K_JOIN .. SIM_K_DEAD (1-7), and
 * val — for SUSPECT / DEAD (value & 0xFFFFFF), the incarnation: the accuser is not part of the identity; for the other kinds
 * the 48 bits that travel (SIM_WIRE_VAL48).  A queued record and a record on the wire with equal (id, val) are the same identity.
 * Identities are ordered by (id, val), ascending.
 *
 * An identity is LIVE in a sample when at least one RUNNING node holds a matching record in its retransmit queue, or a
 * matching record is in the packets in flight — counted on the canonical form SIM_ARR_INBOX: once per fan-out slot mapped to
 * the packet, whether or not the receiver runs (the ledger's and the series' rules).  Only identities of the kinds in
 * kinds_mask are catalogued.
 *
 * Out of scope: sharded handles (every call below returns SIM_ESTATE on one, as the ledger's); more than SIM_CATALOG_LIVE
 * live identities in one sample — such a sample is flagged (word 3), not approximated.
 */
#ifndef SERF_SIM_CATALOG_H
#define SERF_SIM_CATALOG_H

#include <stddef.h>

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_CATALOG_VERSION 1u
#define SIM_CATALOG_LIVE 256u          /* distinct live identities one sample can hold */
#define SIM_CATALOG_MAX 4096u          /* upper bound of max_ids, the registry's size */
#define SIM_CATALOG_MAX_SAMPLES (1u << 20)
#define SIM_CATALOG_SAMPLE_WORDS 48u
#define SIM_CATALOG_RECORD_WORDS 8u
#define SIM_CATALOG_KINDS 0xFEu        /* bits 1-7: every kind */

/* A SAMPLE = 48 unsigned 64-bit words, the state AFTER the sampled tick (what the dumps show when sim_tick == t + 1).  "The
 * previous sample" below is the latest earlier sample of this catalogue whose word 3 is 0; before the first one its set is empty.
 *   0      sim_tick after the tick (t + 1)
 *   1      running nodes
 *   2      distinct live identities of the chosen kinds (0 when word 3 is set)
 *   3      overflow: 1 exactly when the number of distinct live identities of the chosen kinds exceeds SIM_CATALOG_LIVE
 *   4      new: identities appended to the registry by this sample
 *   5      died: live in the previous sample, not live now (whether or not the registry holds them)
 *   6      revived: in the registry before this sample, not live in the previous sample, live now
 *   7      registry size after the sample
 *   8      ids_lost, cumulative: identities that are live now, were not live in the previous sample, are not in the registry
 *          and found it full (one that dies and comes back while the registry is full counts again)
 *   9-12   queued records of running nodes, records in flight, packets in flight with a record, the sum of SIM_META_TRANSMITS
 *          over the queued: ALL kinds, whatever the mask — the ledger's header words 3, 4, 5, 6; exact also when word 3 is set
 *   13-19  distinct live identities of kind 1 .. 7
 *   20-26  queued records of kind 1 .. 7
 *   27-33  records in flight of kind 1 .. 7
 *   34     overflowed samples so far (this one included)
 *   35-47  0
 * Words 13-33 are sums over the live table: the chosen kinds only, 0 in an overflowed sample.  An overflowed sample changes
 * nothing in the registry, is not "the previous sample" of any later one, and its words 4, 5, 6 are 0.
 *
 * The LIVE TABLE of a sample: 8 words per live identity, ascending (id, val), in the ledger's entry layout:
 *   0 id   1 val   2 0   3 holders   4 queued   5 transmits   6 in flight   7 fresh        (include/serf_sim_ledger.h)
 *
 * A REGISTRY RECORD = 8 words.  "now" is word 0 of the sample at hand.
 *   0   id
 *   1   val
 *   2   first seen: word 0 of its first sample (low 32 bits) | last seen: word 0 of its latest sample (high 32 bits)
 *   3   samples in which it was live (low 32 bits) | revivals (high 32 bits)
 *   4   peak queued (low 32 bits) | word 0 of the first sample that reached that peak (high 32 bits)
 *   5   peak holders, with the sample likewise
 *   6   the sum of its in-flight copies over its samples (period 1: the copies the cluster sent, the ledger's word-6 sum)
 *   7   the sum of its queued copies over its samples
 * The registry's order is fixed: identities are appended sample by sample, within one sample in ascending (id, val).  When the
 * registry is full the rest of that sample's new identities and every later new one are counted in ids_lost and not stored.
 *
 * Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_CATALOG_MAX_SAMPLES, kinds_mask == 0 or
 * with a bit outside 1-7, max_ids == 0 or > SIM_CATALOG_MAX, a read beyond `taken`, a list beyond the registry's size, a buffer
 * that is too small; SIM_ESTATE on a sharded handle, between sim_step_begin and sim_step_end, for a start while a catalogue is
 * running and for a read / list / live / stop without one; SIM_ENOMEM when the buffers cannot be allocated.  A call that fails
 * changes nothing. */

/* A sample is taken behind tick t when t >= first_tick, (t - first_tick) % period == 0 and fewer than `capacity` samples have
 * been taken; one that is due with the buffer full is dropped and counted (it does not touch the registry).  A first_tick that
 * has passed already means "now". */
int sim_catalog_start(sim_handle*, uint32_t kinds_mask, uint32_t max_ids, uint32_t first_tick, uint32_t period, uint32_t capacity);
/* Samples taken / dropped so far; waits for nothing.  Both are 0 on a handle without a catalogue. */
int sim_catalog_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken) into out[cap_words]
 * (48 n <= cap_words); *n_out = n. */
int sim_catalog_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Frees the buffers; the samples and the registry are gone. */
int sim_catalog_stop(sim_handle*);
/* Waits for the stream; *total = the registry's size; registry records first .. first + n - 1 — those of them that exist
 * (first <= *total) — into out[cap_words] (8 per record); *n_out = how many. */
int sim_catalog_list(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out, uint32_t* total);
/* Waits for the stream; the live table of the latest sample taken into out[cap_words], *n_out identities: none before the
 * first sample and after an overflowed one. */
int sim_catalog_live(sim_handle*, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* One scan of the state the handle is in now, with or without a running catalogue, which it does not touch: the sample's
 * words into header_out[48] — words 4-8 and 34 are 0: it has no registry — and its live table into live_out[cap_words]
 * (8 * SIM_CATALOG_LIVE words always suffice), *n_out identities. */
int sim_catalog_now(sim_handle*, uint32_t kinds_mask, uint64_t* header_out /* 48 words */, uint64_t* live_out, size_t cap_words,
                    uint32_t* n_out);
uint32_t sim_catalog_version(void);

#ifdef __cplusplus
}
#endif
#endif
