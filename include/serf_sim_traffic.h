/*
 * serf_sim_traffic.h — traffic meter on the device: per node the gossip packets, records and wire units it sent and had
 * addressed to it, accumulated behind the sampled ticks, and per sample how that load was spread over the cluster.
 *
 * The eighth extension of include/serf_sim.h, in the style of include/serf_sim_spread.h: exported by the HIP library
 * (libserf_sim.so) only, with a version of its own (sim_traffic_version), not part of SIM_ABI_VERSION.  The CPU oracle has
 * no meter: it is the checker — every word below is a pure function of the arrays the oracle dumps (SIM_ARR_INBOX /
 * SIM_ARR_ROWS) and of the tick's target draw (tests/traffic_model.py).
 *
 * The series and the ledger give cluster totals of the packets in flight.  The meter says WHICH nodes carry them: under
 * SIM_CF_RANDOM_FANOUT (memberlist's literal kRandomNodes) the in-degree of a node is Poisson-like, under the bijection every
 * node is addressed by exactly the tick's fan-out.  A meter adds no protocol state: digests, events, dumps, checkpoint images
 * do not know it, and a handle without a started meter launches, allocates and synchronises nothing for it.
 *
 * Checkpoints: sim_snapshot holds no meter, sim_restore leaves a running one as it is — its map, its first tick and its
 * period, in absolute ticks (the wording of include/serf_sim_ledger.h).
 *
 * A PACKET OF A SAMPLE, taken behind tick t (now = t + 1): one (sender, fan-out slot) of the canonical SIM_ARR_INBOX with at
 * least one non-empty record, all of its pages taken together.  A packet a sender stored once and mapped to several slots
 * counts once per slot (as in the series and the ledger).  Of a packet:
 *   records   its non-empty records, 1 .. pkt_records
 *   units     the sum of SIM_META_LEN64 over them, in 16-byte units, SIM_PKT_UNITS (87) at most
 *   target    SIM_CF_RANDOM_FANOUT: the k-th node of the sender's draw for tick t (an empty slot has no target and no packet);
 *             the bijection: the fan-out map of tick t
 * Packets that loss removed and packets gossip_to_the_dead skipped were zeroed by their senders: the meter does not see
 * them — "in flight" is "left the node and will arrive".  Probe, ack and push-pull traffic is no packet of the fan-out.
 * RUNNING is SIM_RF_UP after tick t — the state the dumps show when sim_tick == t + 1 —, not the state of the target when the
 * packet is handed to it during tick t + 1.
 *
 * THE MAP: SIM_TRAFFIC_COLUMNS (8) uint32_t per node, cumulative over the samples taken since sim_traffic_start, never
 * cleared while the meter runs; it survives a crash, a revive and a restore:
 *   0  tx_packets   packets the node sent            3  rx_packets   packets addressed to the node
 *   1  tx_records   their records                    4  rx_records   their records
 *   2  tx_units     their units                      5  rx_units     their units
 *   6  rx_peak      the most packets addressed to it in one sample
 *   7  rx_down      packets addressed to it in samples at which it was not running
 * Counters are plain uint32_t additions.  A node sends at most 4 packets of 87 units a sample and SIM_TRAFFIC_MAX_SAMPLES is
 * 2^20: 2^20 * 4 * 87 < 2^32, the tx columns cannot wrap.  The rx columns have no such bound under SIM_CF_RANDOM_FANOUT —
 * any number of senders may draw the same node —: they wrap modulo 2^32 (on average a node is addressed as often as it
 * sends; a wrap takes a node drawn more than ~ 47 times the mean over 2^20 samples).  With a period above 1 the map counts
 * the sampled ticks only.
 *
 * Out of scope: sharded handles (shard_count > 1, SIM_CF_FORCE_SHARDED) — every call below returns SIM_ESTATE on such a
 * handle (vshards > 1 on a handle that holds every node is one handle and is supported); who infected whom (that is include/serf_sim_tree.h).
 */
#ifndef SERF_SIM_TRAFFIC_H
#define SERF_SIM_TRAFFIC_H

#include <stddef.h>

#include "serf_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIM_TRAFFIC_VERSION 1u
#define SIM_TRAFFIC_WORDS 64u              /* words of a sample */
#define SIM_TRAFFIC_MAX_SAMPLES (1u << 20)
#define SIM_TRAFFIC_COLUMNS 8u
#define SIM_TRAFFIC_DEG_BINS 32u           /* in-degree bins of a sample */
#define SIM_TRAFFIC_REC_BINS 16u           /* records-per-packet bins of a sample (= SIM_PKT_RECORDS_MAX) */
#define SIM_TRAFFIC_BINS 32u               /* histogram bins of sim_traffic_summary */
#define SIM_TRAFFIC_SUMMARY_WORDS (8u + SIM_TRAFFIC_BINS)
#define SIM_TRAFFIC_TOP_MAX 64u

/* the columns of the map */
#define SIM_TRAFFIC_TX_PACKETS 0u
#define SIM_TRAFFIC_TX_RECORDS 1u
#define SIM_TRAFFIC_TX_UNITS 2u
#define SIM_TRAFFIC_RX_PACKETS 3u
#define SIM_TRAFFIC_RX_RECORDS 4u
#define SIM_TRAFFIC_RX_UNITS 5u
#define SIM_TRAFFIC_RX_PEAK 6u
#define SIM_TRAFFIC_RX_DOWN 7u

typedef struct sim_traffic_node { uint32_t col[SIM_TRAFFIC_COLUMNS]; } sim_traffic_node;                    /* 32 bytes */
typedef struct sim_traffic_rank { uint32_t id; uint32_t running; sim_traffic_node node; } sim_traffic_rank; /* 40 bytes */

/* A sample = SIM_TRAFFIC_WORDS (64) unsigned 64-bit words, all integers, of the packets in flight AFTER the sampled tick:
 *   0   now: sim_tick after the tick (t + 1)
 *   1   running nodes
 *   2   packets in this sample                       3   their records                  4   their units
 *   5   nodes that sent at least one packet          6   nodes at least one packet is addressed to
 *   7   packets addressed to nodes that are not running
 *   8   the most packets addressed to one node       9   the smallest id with that many; 0 when word 8 is 0
 *   10  the most units addressed to one node         11  the smallest id with that many; 0 when word 10 is 0
 *   12  the most records in one packet               13  the most units in one packet
 *   14  samples accumulated in the map, this one included
 *   15  0
 *   16 + b      nodes, running or not, with min(packets addressed to it in this sample, 31) == b; the bins sum to n_nodes
 *   48 + r - 1  packets with r records, r = 1 .. 16; the bins sum to word 2
 *
 * Errors of all calls: SIM_EINVAL for null pointers, period == 0, capacity == 0 or > SIM_TRAFFIC_MAX_SAMPLES, a read beyond
 * `taken` (or into a buffer that is too small), nodes beyond n_nodes, top_k == 0 or > SIM_TRAFFIC_TOP_MAX, a column above 7,
 * bin_width == 0; SIM_ESTATE on a sharded handle, between sim_step_begin and sim_step_end, for a start while a meter is
 * running and for a read / stop without one; SIM_ENOMEM when the map (n_nodes * 32 bytes), the packet summaries (n_nodes * 8
 * bytes), the sample buffer or a read's scratch cannot be allocated.  Bad arguments are SIM_EINVAL before "no meter" /
 * "already running" is SIM_ESTATE.  A call that fails changes nothing. */

/* A sample is taken — and added to the map — behind tick t (the tick during which sim_tick was t) when t >= first_tick and
 * (t - first_tick) % period == 0 and fewer than `capacity` samples have been taken; one that is due with the buffer full is
 * dropped and counted, and a dropped sample adds nothing to the map — give the buffer the room the run needs.  A first_tick
 * that has passed already means "now" (the handle's tick).  The map starts at zero. */
int sim_traffic_start(sim_handle*, uint32_t first_tick, uint32_t period, uint32_t capacity);
/* Samples taken / dropped so far: the host knows every sampled tick in advance, so this waits for nothing.  Both are 0 on a
 * handle without a meter. */
int sim_traffic_count(const sim_handle*, uint32_t* taken, uint32_t* dropped);
/* Waits for the handle's stream, then copies samples first .. first + n - 1 (first + n <= taken) into out[cap_words]
 * (n * 64 <= cap_words); *n_out = n. */
int sim_traffic_read(sim_handle*, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out);
/* Frees the map and the samples. */
int sim_traffic_stop(sim_handle*);

/* The reads of the map.  Each waits for the handle's stream, computes on the device from the map and the running flags the
 * handle has now, and touches neither the map nor the samples. */

/* The records of nodes first_node .. first_node + count - 1 into out[count] (first_node + count <= n_nodes). */
int sim_traffic_nodes(sim_handle*, uint32_t first_node, uint32_t count, sim_traffic_node* out);
/* top[top_k]: ALL nodes, running or not, ranked by `column` descending, ties by ascending id; `running` is the node's flag
 * now.  Records beyond n_nodes carry id 0xFFFFFFFF and zeros. */
int sim_traffic_top(sim_handle*, uint32_t top_k /* 1 .. 64 */, uint32_t column /* 0 .. 7 */, sim_traffic_rank* top);
/* SIM_TRAFFIC_SUMMARY_WORDS (8 + 32) words of one column over all nodes:
 *   0   column              1   bin_width
 *   2   the sum             3   the max                 4   the smallest id at the max
 *   5   the min             6   nodes with a non-zero value
 *   7   samples accumulated in the map
 *   8 + b   nodes with min(value / bin_width, 31) == b: the last bin takes everything beyond */
int sim_traffic_summary(sim_handle*, uint32_t column, uint32_t bin_width, uint64_t* out /* 8 + 32 words */);
uint32_t sim_traffic_version(void);

#ifdef __cplusplus
}
#endif
#endif
