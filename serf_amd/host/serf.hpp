// serf.hpp — C++ host-side mirror of the reference's `Serf` API (serf-core/src/serf/api.rs) for the
// bulk simulation path, header-only, on top of the C ABI of include/serf_sim.h.
//
// The reference's host language is Rust; this image has no Rust toolchain, so the host above the C
// ABI is C++ (the Rust binding a maintainer would add is in INTEGRATION.md).  Names and argument
// meaning follow the reference: a `Cluster` owns all N simulated nodes (one `Serf::new` each,
// api.rs:25), `Cluster::node(i)` is the `Serf` handle of node i and has the reference's methods.
// Errors: the reference returns `Result<_, Error>` (error.rs:64-81); here a `serf::Error` exception
// carries the SIM_E* code.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <iterator>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/serf_sim.h"
#include "../../include/serf_sim_track.h"
#include "../../include/serf_sim_series.h"
#include "../../include/serf_sim_census.h"
#include "../../include/serf_sim_roll.h"
#include "../../include/serf_sim_ledger.h"
#include "../../include/serf_sim_spread.h"
#include "../../include/serf_sim_traffic.h"
#include "../../include/serf_sim_tree.h"
#include "../../include/serf_sim_qboard.h"
#include "../../include/serf_sim_catalog.h"
#include "../../include/serf_sim_gazette.h"
#include "../../include/serf_sim_detect.h"
#include "wire.hpp"

namespace serf {

struct Error : std::runtime_error {
  int code;
  Error(int c, const char* what) : std::runtime_error(std::string(what) + ": SIM error " + std::to_string(c)), code(c) {}
};
inline void check(int rc, const char* what) {
  if (rc < 0) throw Error(rc, what);
}

// MemberStatus — types/member.rs:54-87
enum class MemberStatus : uint8_t { None = 0, Alive = 1, Leaving = 2, Left = 3, Failed = 4 };
// MemberEventType — event.rs:263-279 (+ user / query events, event.rs:367-378)
enum class EventType : uint32_t { Join = 0, Leave = 1, Failed = 2, Update = 3, Reap = 4, User = 5, Query = 6 };

struct Member {  // types/member.rs:135-185 (id + status; tags/addresses are not on the simulated path)
  uint32_t id;
  MemberStatus status;
  uint64_t status_ltime;
};
using Stats = sim_stats;  // api.rs:586-602
using Event = sim_event;

// Options — options.rs:16-469 (the fields the simulated path reads) + MemberlistOptions::lan()/wan()
struct Options {
  sim_config c{};
  explicit Options(uint32_t n_nodes) {
    c.struct_size = sizeof(sim_config);
    c.n_nodes = n_nodes; c.vshards = 1; c.shard_rank = 0; c.shard_count = 1;
    c.fanout = 3;                                  // lan(): gossip_nodes
    c.view_slots = 0;
    c.event_ring = 512; c.query_ring = 512;        // options.rs:516-517
    c.retransmit_mult = 4; c.probe_interval = 5;   // lan(): 1 s / 200 ms
    c.suspicion_mult = 4; c.suspicion_max_mult = 6; c.indirect_checks = 3;
    c.loss_u32 = 0; c.intent_timeout = 0;
    c.leave_delay = 30;                            // broadcast_timeout 5 s + leave_propagate_delay 1 s
    c.reap_interval = 75;                          // options.rs:506 reap_interval 15 s
    c.reconnect_timeout = c.tombstone_timeout = 432000;  // 24 h (options.rs:507-508)
    c.queue_check_interval = 150; c.max_queue_depth = 4096; c.min_queue_depth = 0;  // options.rs:512-514
    c.push_pull_interval = 150;                    // lan(): 30 s
    c.reconnect_interval = 150;                    // options.rs:507 reconnect_interval 30 s (Reconnector, base.rs:612-681)
    c.ring_overflow = 8;                           // a de-dup bucket is a Vec in the reference (base.rs:801-813): 6 keys + 8 rows of 6 per ring here
    c.flags = SIM_CF_BASELINE_JOINED | SIM_CF_TCP_FALLBACK | SIM_CF_NACKS;  // memberlist lan(): disable_tcp_pings = false, nacks (protocol >= 4)
    c.seed = SIM_DEFAULT_SEED;
  }
  static Options lan(uint32_t n) { return Options(n); }
  static Options wan(uint32_t n) {  // gossip 500 ms, probe 5 s, fan-out 4, suspicion_mult 6 (k capped at 3)
    Options o(n);
    o.c.fanout = 4; o.c.probe_interval = 10; o.c.suspicion_mult = 6;
    return o;
  }
  Options& with_fanout(uint32_t f) { c.fanout = f; return *this; }
  Options& with_view_slots(uint32_t a) { c.view_slots = a; return *this; }
  Options& with_event_buffer_size(uint32_t b) { c.event_ring = b; return *this; }
  Options& with_query_buffer_size(uint32_t b) { c.query_ring = b; return *this; }
  Options& with_packet_loss(double p) { c.loss_u32 = p >= 1.0 ? 0xFFFFFFFFu : (uint32_t)(p * 4294967296.0); return *this; }
  Options& with_disable_tcp_pings(bool off) { c.flags = off ? (c.flags & ~SIM_CF_TCP_FALLBACK) : (c.flags | SIM_CF_TCP_FALLBACK); return *this; }  // memberlist Options::disable_tcp_pings
  Options& with_reconnect_interval(uint32_t ticks) { c.reconnect_interval = ticks; return *this; }  // options.rs:162 (0 = no Reconnector)
  Options& with_ring_overflow(uint32_t rows) { c.ring_overflow = rows; return *this; }  // overflow rows per de-dup ring and node (0: a full bucket treats new keys as seen)
  // handle_prune's wait (serf/base.rs:1628-1653): a pruning leave intent about a Leaving member erases it leave_delay ticks later — the reference's
  // behaviour; off by default (the erase in the tick of the intent), needs the SWIM layer (probe_interval > 0)
  Options& with_prune_wait(bool on) { c.flags = on ? (c.flags | SIM_CF_PRUNE_DELAY) : (c.flags & ~SIM_CF_PRUNE_DELAY); return *this; }
  Options& with_seed(uint64_t s) { c.seed = s; return *this; }
};

class Cluster;

// One simulated node: the reference's `Serf<T, D>` (serf.rs:171-254) for the simulated path.
class Serf {
 public:
  uint32_t local_id() const { return id_; }                                   // api.rs:100
  inline std::vector<Member> members() const;                                 // api.rs:136
  inline Stats stats() const;                                                 // api.rs:150
  inline size_t num_members() const { return stats().members; }               // api.rs:188
  // api.rs:241-299 with the reference's arguments: the size checks before and after encoding (UserEventLimitTooLarge /
  // UserEventTooLarge / RawUserEventTooLarge, error.rs:247-259 -> SIM_ETOOBIG), the message priced by the codec
  // (`encoded_message_len`, wire.hpp) at the node's current event clock; the simulator is told the 32-bit identity of
  // (name, payload) and the framed length.  `max_user_event_size` = options.rs:528 (512), hard limit serf.rs:44 (9 KiB).
  inline void user_event(const std::string& name, const std::vector<uint8_t>& payload, bool coalesce,
                         size_t max_user_event_size = 512);
  // the same with the identity and the length worked out by the caller
  inline void user_event(uint32_t event_key, uint32_t encoded_len = 32, bool coalesce = true);
  inline void query(uint32_t query_id, uint32_t flags = 0);                   // api.rs:304
  // QueryParam.filters (query.rs:37-93, should_process_query query.rs:439-521): `ids` = Filter::Id (at most
  // SIM_QF_IDS), `tag_mask` = the AND of the Filter::Tag masks over tag classes (0xFFFFFFFF = no tag filter)
  inline void query(uint32_t query_id, uint32_t flags, const std::vector<uint32_t>& ids, uint32_t tag_mask = 0xFFFFFFFFu);
  inline void set_tags(uint32_t tag_class);                                   // api.rs:219
  struct QueryStatus { uint64_t acks, responses; bool open; };                // QueryResponse, query.rs:117-303
  inline QueryStatus query_status(uint32_t query_id) const;
  // What the caller of Serf::query holds in the reference (QueryResponse, query.rs:117-236): who acked, who responded and
  // with what, each responder once (the `acks` / `responses` sets of handle_query_response, query.rs:240-303), until the
  // deadline or close().  The simulator tracks the responders (include/serf_sim.h sim_query_responders); a response's
  // PAYLOAD is what the responding node's user hands to respond() — user data, not simulated state — so it comes from the
  // responder function the caller registers (default: empty payloads).  Polling: every call returns the responders that
  // arrived since the previous call, like draining ack_rx / response_rx.
  struct NodeResponse { uint32_t from; std::vector<uint8_t> payload; };       // query.rs:373-385
  class QueryResponse {
   public:
    uint32_t id() const { return id_; }                                       // query.rs:129-133
    bool finished() const;                                                    // query.rs:215-219
    void close() { closed_ = true; }                                          // query.rs:223-237: no further deliveries
    std::vector<uint32_t> acks();                                             // ack_rx (query.rs:203-205)
    std::vector<NodeResponse> responses();                                    // response_rx (query.rs:209-212)
    void on_respond(std::function<std::vector<uint8_t>(uint32_t)> f) { payload_of_ = std::move(f); }
   private:
    friend class Serf;
    QueryResponse(Cluster* c, uint32_t id);   // (below Cluster: it notes the tick the query's deadline cannot outlast)
    std::vector<uint32_t> fresh(int which, std::vector<uint32_t>& seen);
    Cluster* c_;
    uint32_t id_;
    bool closed_ = false;
    mutable bool started_ = false;  // the tracker has been seen under this id (the tick that executes the query has run)
    uint64_t give_up_ = 0;          // a tick by which the query has certainly run out: its tick + 16 * digits10(N) (query.rs:421-427) and some
    std::vector<uint32_t> seen_acks_, seen_resp_;                             // ascending (QueryResponseCore.acks / .responses)
    std::function<std::vector<uint8_t>(uint32_t)> payload_of_;
  };
  // api.rs:304 as the reference shapes it: the query goes out and the caller keeps the QueryResponse
  inline QueryResponse query_response(uint32_t query_id, uint32_t flags = 0) { query(query_id, flags); return QueryResponse(c_, query_id); }
  inline void join(uint32_t peer);                                            // api.rs:318
  // api.rs:366-420: joins through the first of `peers` (memberlist.join_many contacts them in turn and a simulated peer
  // always answers); returns how many were contacted
  inline size_t join_many(const std::vector<uint32_t>& peers) { if (peers.empty()) return 0; join(peers.front()); return 1; }
  inline void leave();                                                        // api.rs:422
  inline void shutdown();                                                     // api.rs:525: the process stops (tests/serf/event.rs:112 shuts a node down)
  inline uint32_t state() const { return stats().serf_state; }                // api.rs:113 SerfState (serf.rs:80-89) as enum sim_serf_state
  inline void remove_failed_node(uint32_t id);                                // api.rs:505
  inline void remove_failed_node_prune(uint32_t id);                          // api.rs:513
  inline void subscribe();                                                    // EventSubscriber, event.rs:430-491

 private:
  friend class Cluster;
  Serf(Cluster* c, uint32_t id) : c_(c), id_(id) {}
  Cluster* c_;
  uint32_t id_;
};

class Cluster {
 public:
  explicit Cluster(const Options& o) : n_(o.c.n_nodes) { check(sim_create(&o.c, &h_), "sim_create"); }
  ~Cluster() { if (h_) sim_destroy(h_); }
  // Options::with_tags for every node at once (start-up tags; include/serf_sim.h sim_init_tags)
  void init_tags(const std::vector<uint8_t>& classes, uint32_t first = 0) {
    check(sim_init_tags(h_, first, (uint32_t)classes.size(), classes.data()), "sim_init_tags");
  }
  Cluster(const Cluster&) = delete;
  Cluster& operator=(const Cluster&) = delete;
  Serf node(uint32_t id) { return Serf(this, id); }
  uint32_t size() const { return n_; }
  void step(uint32_t ticks = 1) { check(sim_step(h_, ticks), "sim_step"); }   // the gossip loop
  void sync() { check(sim_sync(h_), "sim_sync"); }
  uint64_t tick() const { uint64_t t = 0; check(sim_tick(h_, &t), "sim_tick"); return t; }
  // churn / fault injection (the reference tests shutdown() nodes: tests/serf/event.rs:112)
  void crash(uint32_t node, uint64_t at_tick) { check(sim_inject(h_, at_tick, SIM_OP_CRASH, node, 0, 0), "sim_inject"); }
  void revive(uint32_t node, uint64_t at_tick) { check(sim_inject(h_, at_tick, SIM_OP_REVIVE, node, 0, 0), "sim_inject"); }
  std::vector<Event> drain_events() {
    std::vector<Event> ev(1 << 16);
    uint32_t n = 0;
    check(sim_drain_events(h_, ev.data(), (uint32_t)ev.size(), &n), "sim_drain_events");
    ev.resize(n);
    return ev;
  }
  // fraction of running nodes that have applied the rumour (rounds-to-99 % = first tick >= 0.99)
  double convergence(uint32_t kind, uint32_t key, uint64_t ltime) {
    uint64_t seen = 0, up = 0;
    check(sim_convergence(h_, kind, key, ltime, &seen, &up), "sim_convergence");
    return up ? (double)seen / (double)up : 0.0;
  }
  // device-resident trackers (include/serf_sim_track.h): dissemination / detection latency without a poll per tick — register,
  // step(n) with n as large as the run, read.  HIP library only (the CPU oracle exports no sim_track_*).
  std::vector<uint32_t> track_add(const std::vector<sim_tracker>& t) {
    std::vector<uint32_t> ids(t.size());
    check(sim_track_add(h_, t.data(), (uint32_t)t.size(), ids.data()), "sim_track_add");
    return ids;
  }
  void track_remove(const std::vector<uint32_t>& ids) { check(sim_track_remove(h_, ids.data(), (uint32_t)ids.size()), "sim_track_remove"); }
  std::vector<sim_track_result> track_read(const std::vector<uint32_t>& ids) {
    std::vector<sim_track_result> out(ids.size());
    check(sim_track_read(h_, ids.data(), (uint32_t)ids.size(), out.data()), "sim_track_read");
    return out;
  }
  std::pair<uint32_t, uint32_t> track_active() {  // (registered, of which not retired)
    uint32_t r = 0, a = 0;
    check(sim_track_active(h_, &r, &a), "sim_track_active");
    return {r, a};
  }
  static sim_tracker rumour_tracker(uint32_t kind, uint32_t key, uint64_t ltime, uint32_t start = 0, uint32_t max_age = 0) {
    return sim_tracker{SIM_TRK_RUMOUR, kind, key, 0, ltime, start, max_age};
  }
  static sim_tracker member_tracker(uint32_t subject, uint32_t status_mask, uint32_t swim_mask = 0, uint32_t min_inc = 0,
                                    uint32_t start = 0, uint32_t max_age = 0) {
    return sim_tracker{SIM_TRK_MEMBER, subject, (status_mask & 0xFFu) | (swim_mask << 8), min_inc, 0, start, max_age};
  }
  // device-resident time series (include/serf_sim_series.h): one sample of cluster gauges (queue depths by class and as a histogram,
  // health scores, suspicion timers, clock spread, what the packets in flight carry) behind every period-th tick — start,
  // step(n) with n as large as the run, read.  HIP library only (the CPU oracle exports no sim_series_*).
  void series_start(uint32_t first_tick = 0, uint32_t period = 1, uint32_t capacity = 1u << 16) {
    check(sim_series_start(h_, first_tick, period, capacity), "sim_series_start");
  }
  // (samples taken, dropped with the buffer full); waits for nothing
  std::pair<uint32_t, uint32_t> series_count() const { return sample_count(sim_series_count, "sim_series_count"); }
  std::vector<sim_series_sample> series_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    if (n == 0xFFFFFFFFu) { const uint32_t t = series_count().first; n = t > first ? t - first : 0; }
    std::vector<sim_series_sample> out(n ? n : 1);
    uint32_t got = 0;
    check(sim_series_read(h_, first, n, out.data(), &got), "sim_series_read");
    out.resize(got);
    return out;
  }
  void series_stop() { check(sim_series_stop(h_), "sim_series_stop"); }
  // membership census (include/serf_sim_census.h): behind every period-th tick one record per subject that owns a view slot — how
  // many running nodes hold it Alive / Leaving / Left / Failed, Suspect / Dead, at which Lamport times and incarnations — and a
  // header of cluster-wide figures (settled subjects, false positives, undetected failures).  HIP library only.
  struct CensusSample {
    sim_census_header header;
    std::vector<sim_census_subject> subjects;  // header.w[3] of them, in slot order
  };
  void census_start(uint32_t first_tick = 0, uint32_t period = 1, uint32_t capacity = 1u << 12, uint32_t max_subjects = 64) {
    check(sim_census_start(h_, first_tick, period, capacity, max_subjects), "sim_census_start");
    census_max_ = max_subjects;
  }
  // (samples taken, dropped with the buffer full); waits for nothing
  std::pair<uint32_t, uint32_t> census_count() const { return sample_count(sim_census_count, "sim_census_count"); }
  std::vector<CensusSample> census_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    return sample_read<CensusSample>(sim_census_count, sim_census_read, "sim_census", first, n, ((size_t)census_max_ + 1) * SIM_CENSUS_WORDS,
                                     [](const uint64_t* w, CensusSample& s) { unpack(w, (size_t)w[3], s.header, s.subjects); });
  }
  void census_stop() { check(sim_census_stop(h_), "sim_census_stop"); }
  CensusSample census_now(uint32_t cap = 64) {  // the state the handle is in now, with or without a running census
    CensusSample s;
    s.subjects.resize(cap ? cap : 1);
    uint32_t got = 0;
    check(sim_census_now(h_, &s.header, s.subjects.data(), cap, &got), "sim_census_now");
    s.subjects.resize(got);
    return s;
  }
  // observer roll (include/serf_sim_roll.h): behind every period-th tick a header over the running nodes — how many subjects they
  // do not know or know at an older time than somebody else, how many running members they hold Failed or Suspect, how many
  // stopped ones Alive, as sums, maxima and a histogram — and the top_k worst of them by `rank_by`.  HIP library only.
  struct RollSample {
    sim_roll_header header;
    std::vector<sim_roll_node> top;    // the listed ones (header.w[3] & 0xFFFFFFFF of them): descending score, ties in ascending id
    std::vector<sim_roll_node> nodes;  // roll_now(.., true) only: every node's record, in id order
  };
  void roll_start(uint32_t first_tick = 0, uint32_t period = 1, uint32_t capacity = 1u << 12, uint32_t top_k = 8,
                  uint32_t rank_by = SIM_ROLL_BY_STALE) {
    check(sim_roll_start(h_, first_tick, period, capacity, top_k, rank_by), "sim_roll_start");
    roll_top_ = top_k;
  }
  // (samples taken, dropped with the buffer full); waits for nothing
  std::pair<uint32_t, uint32_t> roll_count() const { return sample_count(sim_roll_count, "sim_roll_count"); }
  std::vector<RollSample> roll_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    return sample_read<RollSample>(sim_roll_count, sim_roll_read, "sim_roll", first, n, SIM_ROLL_HEADER_WORDS + (size_t)roll_top_ * SIM_ROLL_NODE_WORDS,
                                   [](const uint64_t* w, RollSample& s) { unpack(w, (size_t)(w[3] & 0xFFFFFFFFu), s.header, s.top); });
  }
  void roll_stop() { check(sim_roll_stop(h_), "sim_roll_stop"); }
  // the state the handle is in now, with or without a running roll
  RollSample roll_now(uint32_t top_k = 8, uint32_t rank_by = SIM_ROLL_BY_STALE, bool nodes = false) {
    RollSample s;
    s.top.resize(top_k ? top_k : 1);
    if (nodes) s.nodes.resize(n_);
    check(sim_roll_now(h_, top_k, rank_by, &s.header, s.top.data(), nodes ? s.nodes.data() : nullptr), "sim_roll_now");
    s.top.resize((size_t)(s.header.w[3] & 0xFFFFFFFFu));
    return s;
  }
  // rumour ledger (include/serf_sim_ledger.h): behind every period-th tick, for each of up to 64 record identities (kind, key, val),
  // how many running nodes have applied the rumour, how many hold it in their queues, the copies queued and their transmits, the
  // copies in flight and the fresh ones — what a rumour costs and when it dies.  HIP library only.
  struct LedgerSample {
    uint64_t header[SIM_LEDGER_HEADER_WORDS];  // tick, running, n, queued, in flight, packets, transmits, 0
    struct Entry { uint64_t id, val, reach, holders, queued, transmits, in_flight, fresh; };  // id = key | kind << 32
    std::vector<Entry> entries;                // in the order they were given
  };
  void ledger_start(const std::vector<sim_ledger_entry>& e, uint32_t first_tick = 0, uint32_t period = 1, uint32_t capacity = 1u << 12) {
    check(sim_ledger_start(h_, e.data(), (uint32_t)e.size(), first_tick, period, capacity), "sim_ledger_start");
    ledger_n_ = (uint32_t)e.size();
  }
  // (samples taken, dropped with the buffer full); waits for nothing
  std::pair<uint32_t, uint32_t> ledger_count() const { return sample_count(sim_ledger_count, "sim_ledger_count"); }
  std::vector<LedgerSample> ledger_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    const uint32_t ne = ledger_n_;
    return sample_read<LedgerSample>(sim_ledger_count, sim_ledger_read, "sim_ledger", first, n, SIM_LEDGER_HEADER_WORDS + (size_t)ne * SIM_LEDGER_ENTRY_WORDS,
                                     [ne](const uint64_t* w, LedgerSample& s) { unpack(w, ne, s.header, s.entries); });
  }
  void ledger_stop() { check(sim_ledger_stop(h_), "sim_ledger_stop"); }
  // the state the handle is in now, with or without a running ledger, for entries of its own
  LedgerSample ledger_now(const std::vector<sim_ledger_entry>& e) {
    std::vector<uint64_t> words(SIM_LEDGER_HEADER_WORDS + (e.size() ? e.size() : 1) * SIM_LEDGER_ENTRY_WORDS);
    check(sim_ledger_now(h_, e.data(), (uint32_t)e.size(), words.data()), "sim_ledger_now");
    LedgerSample s;
    unpack(words.data(), e.size(), s.header, s.entries);
    return s;
  }
  // detection log (include/serf_sim_detect.h): behind every period-th tick every view slot's subject is judged — down (when was
  // the crash first suspected, when did half, 99 % and all of the running nodes know) or running and accused (how far did it get, was
  // it refuted) — a sample is a header of cumulative figures, the episodes that closed are appended to a log.  HIP library only.
  void detect_start(uint32_t first_tick = 0, uint32_t period = 1, uint32_t capacity = 1u << 12, uint32_t log_capacity = 1u << 16) {
    check(sim_detect_start(h_, first_tick, period, capacity, log_capacity), "sim_detect_start");
  }
  // (samples taken, dropped with the buffer full); waits for nothing
  std::pair<uint32_t, uint32_t> detect_count() const { return sample_count(sim_detect_count, "sim_detect_count"); }
  std::vector<sim_detect_header> detect_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    return sample_read<sim_detect_header>(sim_detect_count, sim_detect_read, "sim_detect", first, n, SIM_DETECT_WORDS,
                                          [](const uint64_t* w, sim_detect_header& s) { std::memcpy(&s, w, sizeof s); });
  }
  // (log records written, lost with the log full); waits for the handle's stream
  std::pair<uint64_t, uint64_t> detect_log_count() {
    uint64_t w = 0, l = 0;
    check(sim_detect_log_count(h_, &w, &l), "sim_detect_log_count");
    return {w, l};
  }
  // the episodes that have closed, in (sample, ascending slot) order (default: all from `first` on)
  std::vector<sim_detect_episode> detect_log(uint64_t first = 0, uint32_t n = 0xFFFFFFFFu) {
    if (n == 0xFFFFFFFFu) { const uint64_t w = detect_log_count().first; n = w > first ? (uint32_t)(w - first) : 0; }
    std::vector<sim_detect_episode> out(n ? n : 1);
    uint32_t got = 0;
    check(sim_detect_log_read(h_, first, n, out.data(), (uint32_t)out.size(), &got), "sim_detect_log_read");
    out.resize(got);
    return out;
  }
  // the episodes still open, in ascending slot order (a slot each: there are no more than nodes)
  std::vector<sim_detect_episode> detect_open() {
    std::vector<sim_detect_episode> out(n_);
    uint32_t got = 0;
    check(sim_detect_open(h_, out.data(), n_, &got), "sim_detect_open");
    out.resize(got);
    return out;
  }
  void detect_stop() { check(sim_detect_stop(h_), "sim_detect_stop"); }
  // spread map (include/serf_sim_spread.h): behind every period-th tick every running node that has applied one of up to 64
  // rumours (kind 1-4, key, ltime) and has no arrival for it yet gets arrival = tick + 1 — which nodes got a rumour late or never,
  // and when each node got it.  A sample says what it latched and where each entry stands; the map is read by entry (spread_map),
  // summed up (spread_summary), by its gaps (spread_unreached) or by node (spread_late).  HIP library only.
  struct SpreadSample {
    uint64_t header[SIM_SPREAD_HEADER_WORDS];  // now, running, n, latched now, entries started, entries everybody running has, 0, 0
    struct Entry { uint64_t id, val, latched, reached, reached_up, holds, first, last; };  // id = key | kind << 32
    std::vector<Entry> entries;                // in the order they were given
  };
  struct SpreadSummary { uint64_t id, val, first, last, reached, reached_up, unreached_up, late_sum, bins[SIM_SPREAD_BINS]; };
  struct SpreadLate {
    std::vector<sim_spread_node> top;    // the worst running nodes, worst first; records beyond the running nodes are zero
    std::vector<sim_spread_node> nodes;  // every node's record, when asked for
  };
  void spread_start(const std::vector<sim_spread_entry>& e, uint32_t first_tick = 0, uint32_t period = 1, uint32_t capacity = 1u << 12) {
    check(sim_spread_start(h_, e.data(), (uint32_t)e.size(), first_tick, period, capacity), "sim_spread_start");
    spread_n_ = (uint32_t)e.size();
  }
  // (samples taken, dropped with the buffer full); waits for nothing
  std::pair<uint32_t, uint32_t> spread_count() const { return sample_count(sim_spread_count, "sim_spread_count"); }
  std::vector<SpreadSample> spread_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    const uint32_t ne = spread_n_;
    return sample_read<SpreadSample>(sim_spread_count, sim_spread_read, "sim_spread", first, n, SIM_SPREAD_HEADER_WORDS + (size_t)ne * SIM_SPREAD_ENTRY_WORDS,
                                     [ne](const uint64_t* w, SpreadSample& s) { unpack(w, ne, s.header, s.entries); });
  }
  void spread_stop() { check(sim_spread_stop(h_), "sim_spread_stop"); }
  // arrival[entry][first_node ..]: 0 = not yet (default: up to the last node)
  std::vector<uint32_t> spread_map(uint32_t entry, uint32_t first_node = 0, uint32_t count = 0xFFFFFFFFu) {
    if (count == 0xFFFFFFFFu) count = n_ > first_node ? n_ - first_node : 0;
    std::vector<uint32_t> out(count ? count : 1);
    check(sim_spread_map(h_, entry, first_node, count, out.data()), "sim_spread_map");
    out.resize(count);
    return out;
  }
  std::vector<SpreadSummary> spread_summary(uint32_t bin_width = 1) {
    std::vector<SpreadSummary> out(spread_n_ ? spread_n_ : 1);
    check(sim_spread_summary(h_, bin_width, reinterpret_cast<uint64_t*>(out.data())), "sim_spread_summary");
    out.resize(spread_n_);
    return out;
  }
  // (the running nodes without an arrival for `entry` in ascending id, the first `cap` of them; the number of all of them)
  std::pair<std::vector<uint32_t>, uint32_t> spread_unreached(uint32_t entry, uint32_t cap = 0xFFFFFFFFu) {
    if (cap > n_) cap = n_;
    std::vector<uint32_t> ids(cap ? cap : 1);
    uint32_t got = 0, total = 0;
    check(sim_spread_unreached(h_, entry, ids.data(), cap, &got, &total), "sim_spread_unreached");
    ids.resize(got);
    return {ids, total};
  }
  SpreadLate spread_late(uint32_t top_k = 8, uint32_t rank_by = SIM_SPREAD_BY_MISSED, bool nodes = false) {
    SpreadLate s;
    s.top.resize(top_k ? top_k : 1);
    if (nodes) s.nodes.resize(n_);
    check(sim_spread_late(h_, top_k, rank_by, s.top.data(), nodes ? s.nodes.data() : nullptr), "sim_spread_late");
    s.top.resize(top_k);
    return s;
  }
  // traffic meter (include/serf_sim_traffic.h): behind every period-th tick the gossip packets in flight are counted per sender and per
  // target — packets, records, 16-byte units — into a map of eight uint32_t a node, and a sample says how the load was spread: the
  // in-degree histogram, the most addressed node, what went to stopped processes.  The map is read by node (traffic_nodes), ranked
  // (traffic_top) or summed up by column (traffic_summary).  HIP library only.
  struct TrafficSample { uint64_t w[SIM_TRAFFIC_WORDS]; };   // the table of include/serf_sim_traffic.h
  struct TrafficSummary { uint64_t column, bin_width, sum, max, max_id, min, nonzero, samples, bins[SIM_TRAFFIC_BINS]; };
  void traffic_start(uint32_t first_tick = 0, uint32_t period = 1, uint32_t capacity = 1u << 12) {
    check(sim_traffic_start(h_, first_tick, period, capacity), "sim_traffic_start");
  }
  // (samples taken, dropped with the buffer full); waits for nothing
  std::pair<uint32_t, uint32_t> traffic_count() const { return sample_count(sim_traffic_count, "sim_traffic_count"); }
  std::vector<TrafficSample> traffic_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    return sample_read<TrafficSample>(sim_traffic_count, sim_traffic_read, "sim_traffic", first, n, SIM_TRAFFIC_WORDS,
                                      [](const uint64_t* w, TrafficSample& s) { std::memcpy(&s, w, sizeof s); });
  }
  void traffic_stop() { check(sim_traffic_stop(h_), "sim_traffic_stop"); }
  // the map's records of nodes first_node .. (default: up to the last node)
  std::vector<sim_traffic_node> traffic_nodes(uint32_t first_node = 0, uint32_t count = 0xFFFFFFFFu) {
    if (count == 0xFFFFFFFFu) count = n_ > first_node ? n_ - first_node : 0;
    std::vector<sim_traffic_node> out(count ? count : 1);
    check(sim_traffic_nodes(h_, first_node, count, out.data()), "sim_traffic_nodes");
    out.resize(count);
    return out;
  }
  // ALL nodes ranked by a column (SIM_TRAFFIC_TX_PACKETS .. SIM_TRAFFIC_RX_DOWN) descending, ties by ascending id: the first top_k
  std::vector<sim_traffic_rank> traffic_top(uint32_t top_k = 10, uint32_t column = SIM_TRAFFIC_RX_UNITS) {
    std::vector<sim_traffic_rank> out(top_k ? top_k : 1);
    check(sim_traffic_top(h_, top_k, column, out.data()), "sim_traffic_top");
    out.resize(top_k);
    return out;
  }
  TrafficSummary traffic_summary(uint32_t column = SIM_TRAFFIC_RX_UNITS, uint32_t bin_width = 1) {
    TrafficSummary s;
    check(sim_traffic_summary(h_, column, bin_width, reinterpret_cast<uint64_t*>(&s)), "sim_traffic_summary");
    return s;
  }
  // rumour tree (include/serf_sim_tree.h): behind every tick every running node that has applied one of up to 64 rumours and has no
  // arrival for it yet gets arrival = tick + 1, as its parent the smallest sender among the packets with the rumour that the sample
  // before saw addressed to it, and hop = the parent's + 1 (an orphan, hop 0, without one) — who infected whom.  A sample says what
  // it latched, how many copies travel and how many of them are still useful; the tree is read by node (tree_links), summed up
  // (tree_summary), by chain (tree_path) or ranked by children (tree_top).  HIP library only.
  struct TreeSample {
    uint64_t header[SIM_TREE_HEADER_WORDS];  // now, running, n, latched now, of them orphans, copies in flight, fresh carriers, 0
    struct Entry { uint64_t id, val, latched, new_orphans, reached, orphans, copies, fresh; };  // id = key | kind << 32
    std::vector<Entry> entries;              // in the order they were given
  };
  struct TreeSummary {
    uint64_t id, val, reached, orphans, depth, hop_sum, most_children, most_children_id, hop_bins[SIM_TREE_BINS], children_bins[SIM_TREE_BINS];
  };
  void tree_start(const std::vector<sim_tree_entry>& e, uint32_t first_tick = 0, uint32_t capacity = 1u << 12) {
    check(sim_tree_start(h_, e.data(), (uint32_t)e.size(), first_tick, capacity), "sim_tree_start");
    tree_n_ = (uint32_t)e.size();
  }
  // (samples taken, dropped with the buffer full); waits for nothing
  std::pair<uint32_t, uint32_t> tree_count() const { return sample_count(sim_tree_count, "sim_tree_count"); }
  std::vector<TreeSample> tree_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    const uint32_t ne = tree_n_;
    return sample_read<TreeSample>(sim_tree_count, sim_tree_read, "sim_tree", first, n, SIM_TREE_HEADER_WORDS + (size_t)ne * SIM_TREE_ENTRY_WORDS,
                                   [ne](const uint64_t* w, TreeSample& s) { unpack(w, ne, s.header, s.entries); });
  }
  void tree_stop() { check(sim_tree_stop(h_), "sim_tree_stop"); }
  // {arrival, parent, hop, children} of nodes first_node .. in the tree of `entry` (default: up to the last node)
  std::vector<sim_tree_link> tree_links(uint32_t entry, uint32_t first_node = 0, uint32_t count = 0xFFFFFFFFu) {
    if (count == 0xFFFFFFFFu) count = n_ > first_node ? n_ - first_node : 0;
    std::vector<sim_tree_link> out(count ? count : 1);
    check(sim_tree_links(h_, entry, first_node, count, out.data()), "sim_tree_links");
    out.resize(count);
    return out;
  }
  std::vector<TreeSummary> tree_summary() {
    std::vector<TreeSummary> out(tree_n_ ? tree_n_ : 1);
    check(sim_tree_summary(h_, reinterpret_cast<uint64_t*>(out.data())), "sim_tree_summary");
    out.resize(tree_n_);
    return out;
  }
  // (the chain node, parent, grandparent ... up to its orphan, the first `cap` ids; its length hop + 1, 0 without an arrival)
  std::pair<std::vector<uint32_t>, uint32_t> tree_path(uint32_t entry, uint32_t node, uint32_t cap = 0xFFFFFFFFu) {
    if (cap > n_) cap = n_;
    std::vector<uint32_t> ids(cap ? cap : 1);
    uint32_t got = 0, total = 0;
    check(sim_tree_path(h_, entry, node, ids.data(), cap, &got, &total), "sim_tree_path");
    ids.resize(got);
    return {ids, total};
  }
  // ALL nodes ranked by their children in the tree of `entry` descending, ties by ascending id: the first top_k
  std::vector<sim_tree_rank> tree_top(uint32_t entry, uint32_t top_k = 10) {
    std::vector<sim_tree_rank> out(top_k ? top_k : 1);
    check(sim_tree_top(h_, entry, top_k, out.data()), "sim_tree_top");
    out.resize(top_k);
    return out;
  }
  // query board (include/serf_sim_qboard.h): behind every period-th tick, for up to 64 query ids — running or not yet — the acks and
  // responses their origins hold, how many of the nodes the filters admit run, have answered, stay silent, and the ticks at which a
  // first / half / 90 % / 99 % / all of them had answered: what `while (!r.finished()) step(), r.acks()` polls, without a poll.  The
  // board is read by entry (qboard_silent: who stayed silent), by node (qboard_nodes) or ranked (qboard_top); qboard_now is the bulk
  // form of query_status and needs no board.  HIP library only.
  struct QBoardSample {
    uint64_t header[SIM_QBOARD_HEADER_WORDS];  // now, running, n, entries open / closed / waiting / displaced, new acks + responses
    struct Entry {
      uint32_t id, state, origin, flags;
      uint64_t deadline, acks, responses, eligible, answered, responded, silent, new_acks, new_responses, t_first, t_half, t_90, t_99, t_all;
    };
    std::vector<Entry> entries;
  };
  struct QBoardTop { std::vector<sim_qboard_node> top, nodes; };  // nodes: every node's record, when asked for
  void qboard_start(const std::vector<uint32_t>& ids, uint32_t first_tick = 0, uint32_t period = 1, uint32_t capacity = 1u << 12) {
    check(sim_qboard_start(h_, ids.data(), (uint32_t)ids.size(), first_tick, period, capacity), "sim_qboard_start");
    qboard_n_ = (uint32_t)ids.size();
  }
  // (samples taken, dropped with the buffer full); waits for nothing
  std::pair<uint32_t, uint32_t> qboard_count() const { return sample_count(sim_qboard_count, "sim_qboard_count"); }
  std::vector<QBoardSample> qboard_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    const uint32_t ne = qboard_n_;
    return sample_read<QBoardSample>(sim_qboard_count, sim_qboard_read, "sim_qboard", first, n,
                                     SIM_QBOARD_HEADER_WORDS + (size_t)ne * SIM_QBOARD_ENTRY_WORDS,
                                     [ne](const uint64_t* w, QBoardSample& s) { unpack(w, ne, s.header, s.entries); });
  }
  void qboard_stop() { check(sim_qboard_stop(h_), "sim_qboard_stop"); }
  // one stateless sample of ids of the caller's own, with or without a running board (latches and `new` are 0)
  QBoardSample qboard_now(const std::vector<uint32_t>& ids) {
    std::vector<uint64_t> w(SIM_QBOARD_HEADER_WORDS + (ids.size() ? ids.size() : 1) * SIM_QBOARD_ENTRY_WORDS);
    check(sim_qboard_now(h_, ids.data(), (uint32_t)ids.size(), w.data()), "sim_qboard_now");
    QBoardSample s;
    unpack(w.data(), ids.size(), s.header, s.entries);
    return s;
  }
  // (the eligible nodes of `entry` without the ack (which 0) / response (which 1) bit in ascending id, the first `cap`; the number of all)
  std::pair<std::vector<uint32_t>, uint32_t> qboard_silent(uint32_t entry, uint32_t which = 0, uint32_t cap = 0xFFFFFFFFu) {
    if (cap > n_) cap = n_;
    std::vector<uint32_t> ids(cap ? cap : 1);
    uint32_t got = 0, total = 0;
    check(sim_qboard_silent(h_, entry, which, ids.data(), cap, &got, &total), "sim_qboard_silent");
    ids.resize(got);
    return {ids, total};
  }
  // the records of nodes first_node .. (default: up to the last node) over the entries that own their table entry now
  std::vector<sim_qboard_node> qboard_nodes(uint32_t first_node = 0, uint32_t count = 0xFFFFFFFFu) {
    if (count == 0xFFFFFFFFu) count = n_ > first_node ? n_ - first_node : 0;
    std::vector<sim_qboard_node> out(count ? count : 1);
    check(sim_qboard_nodes(h_, first_node, count, out.data()), "sim_qboard_nodes");
    out.resize(count);
    return out;
  }
  QBoardTop qboard_top(uint32_t top_k = 8, uint32_t rank_by = SIM_QBOARD_BY_SILENT_ACK, bool nodes = false) {
    QBoardTop s;
    s.top.resize(top_k ? top_k : 1);
    if (nodes) s.nodes.resize(n_);
    check(sim_qboard_top(h_, top_k, rank_by, s.top.data(), nodes ? s.nodes.data() : nullptr), "sim_qboard_top");
    s.top.resize(top_k);
    return s;
  }
  // rumour catalogue (include/serf_sim_catalog.h): behind every period-th tick the record identities that are LIVE — queued at a
  // running node or in a packet in flight — are found, not named: a sample of 48 words, the live table of the latest sample and a
  // registry of every identity ever found (first and last seen, peaks, the copies it cost).  Feed what it lists to the ledger, the
  // spread map or the tree.
  struct CatalogSample { uint64_t w[SIM_CATALOG_SAMPLE_WORDS]; };  // the words of the header's table
  struct CatalogLive { uint64_t id, val, reserved, holders, queued, transmits, in_flight, fresh; };  // the ledger's entry layout
  struct CatalogRecord {
    uint64_t id, val;
    uint32_t first_seen, last_seen, samples, revivals, peak_queued, peak_queued_at, peak_holders, peak_holders_at;
    uint64_t in_flight_sum, queued_sum;
    uint32_t kind() const { return (uint32_t)(id >> 32); }
    uint32_t key() const { return (uint32_t)id; }
  };
  struct CatalogNow { CatalogSample sample; std::vector<CatalogLive> live; };
  void catalog_start(uint32_t kinds_mask = SIM_CATALOG_KINDS, uint32_t max_ids = SIM_CATALOG_MAX, uint32_t first_tick = 0, uint32_t period = 1,
                     uint32_t capacity = 1u << 12) {
    check(sim_catalog_start(h_, kinds_mask, max_ids, first_tick, period, capacity), "sim_catalog_start");
  }
  std::pair<uint32_t, uint32_t> catalog_count() const { return sample_count(sim_catalog_count, "sim_catalog_count"); }
  std::vector<CatalogSample> catalog_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    return sample_read<CatalogSample>(sim_catalog_count, sim_catalog_read, "sim_catalog", first, n, SIM_CATALOG_SAMPLE_WORDS,
                                      [](const uint64_t* w, CatalogSample& s) { std::memcpy(s.w, w, sizeof s.w); });
  }
  void catalog_stop() { check(sim_catalog_stop(h_), "sim_catalog_stop"); }
  // registry records first .. first + n - 1 (default: up to the last), in the registry's fixed order
  std::vector<CatalogRecord> catalog_list(uint32_t first = 0, uint32_t n = SIM_CATALOG_MAX) {
    std::vector<CatalogRecord> out(n ? n : 1);
    uint32_t got = 0, total = 0;
    check(sim_catalog_list(h_, first, n, reinterpret_cast<uint64_t*>(out.data()), out.size() * SIM_CATALOG_RECORD_WORDS, &got, &total), "sim_catalog_list");
    out.resize(got);
    return out;
  }
  // the live table of the latest sample, ascending (id, val); empty before the first sample and after an overflowed one
  std::vector<CatalogLive> catalog_live() {
    std::vector<CatalogLive> out(SIM_CATALOG_LIVE);
    uint32_t got = 0;
    check(sim_catalog_live(h_, reinterpret_cast<uint64_t*>(out.data()), out.size() * 8, &got), "sim_catalog_live");
    out.resize(got);
    return out;
  }
  // one scan of the state the handle is in now, with or without a running catalogue, which it does not touch
  CatalogNow catalog_now(uint32_t kinds_mask = SIM_CATALOG_KINDS) {
    CatalogNow s;
    s.live.resize(SIM_CATALOG_LIVE);
    uint32_t got = 0;
    check(sim_catalog_now(h_, kinds_mask, s.sample.w, reinterpret_cast<uint64_t*>(s.live.data()), s.live.size() * 8, &got), "sim_catalog_now");
    s.live.resize(got);
    return s;
  }
  // member gazette (include/serf_sim_gazette.h): every node's member events — Join / Leave / Failed / Reap, flaps, suspicions raised and
  // cleared — counted per node and per subject by diffing every view entry's bits against the previous sample's, behind every period-th
  // tick: a sample of 64 words, a node map and a subject map of eight columns a row (SIM_GAZETTE_JOIN ..), read whole, in slices or ranked.
  struct GazetteSample { uint64_t w[SIM_GAZETTE_WORDS]; };  // the words of the header's table
  void gazette_start(uint32_t first_tick = 0, uint32_t period = 1, uint32_t capacity = 1u << 12, uint32_t flap_window = 60) {
    check(sim_gazette_start(h_, first_tick, period, capacity, flap_window), "sim_gazette_start");
  }
  std::pair<uint32_t, uint32_t> gazette_count() const { return sample_count(sim_gazette_count, "sim_gazette_count"); }
  std::vector<GazetteSample> gazette_read(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) {  // (default: all from `first` on)
    return sample_read<GazetteSample>(sim_gazette_count, sim_gazette_read, "sim_gazette", first, n, SIM_GAZETTE_WORDS,
                                      [](const uint64_t* w, GazetteSample& s) { std::memcpy(s.w, w, sizeof s.w); });
  }
  // rows first .. first + n - 1 of the node map / the subject map (default: up to the last node)
  std::vector<sim_gazette_row> gazette_nodes(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) { return gazette_rows(sim_gazette_nodes, "sim_gazette_nodes", first, n); }
  std::vector<sim_gazette_row> gazette_subjects(uint32_t first = 0, uint32_t n = 0xFFFFFFFFu) { return gazette_rows(sim_gazette_subjects, "sim_gazette_subjects", first, n); }
  // ALL rows of a map ranked by a column, descending, ties in ascending id: the first k
  std::vector<sim_gazette_rank> gazette_top(uint32_t map = SIM_GAZETTE_MAP_NODES, uint32_t column = SIM_GAZETTE_FAILED, uint32_t k = 10) {
    std::vector<sim_gazette_rank> out(k ? k : 1);
    check(sim_gazette_top(h_, map, column, k, out.data()), "sim_gazette_top");
    out.resize(k);
    return out;
  }
  void gazette_stop() { check(sim_gazette_stop(h_), "sim_gazette_stop"); }
  // checkpoint / resume (canonical image; snapshot.rs:117-126,228-347 is the per-node analogue)
  std::vector<uint8_t> snapshot() {
    size_t n = 0;
    check(sim_snapshot(h_, nullptr, 0, &n), "sim_snapshot");
    std::vector<uint8_t> img(n);
    check(sim_snapshot(h_, img.data(), img.size(), &n), "sim_snapshot");
    return img;
  }
  void restore(const std::vector<uint8_t>& img) { check(sim_restore(h_, img.data(), img.size()), "sim_restore"); }
  sim_handle* raw() { return h_; }

 private:
  sim_handle* h_ = nullptr;
  uint32_t n_;
  uint32_t census_max_ = 1;  // max_subjects of the running census: the stride of its samples
  uint32_t roll_top_ = 1;    // top_k of the running roll: likewise
  uint32_t ledger_n_ = 1;    // entries of the running ledger: likewise
  uint32_t spread_n_ = 1;    // entries of the running spread map: likewise
  uint32_t tree_n_ = 1;      // entries of the running rumour tree: likewise
  uint32_t qboard_n_ = 1;    // entries of the running query board: likewise
  static_assert(sizeof(QBoardSample::Entry) == 8 * SIM_QBOARD_ENTRY_WORDS, "an entry's record is sixteen words");
  static_assert(sizeof(CatalogLive) == 64 && sizeof(CatalogRecord) == 8 * SIM_CATALOG_RECORD_WORDS && sizeof(CatalogSample) == 8 * SIM_CATALOG_SAMPLE_WORDS,
                "a live identity and a registry record are eight words, a sample forty-eight");
  static_assert(sizeof(TreeSample::Entry) == 8 * SIM_TREE_ENTRY_WORDS && sizeof(TreeSummary) == 8 * SIM_TREE_SUMMARY_WORDS,
                "an entry's record is eight words, its summary seventy-two");
  static_assert(sizeof(SpreadSample::Entry) == 8 * SIM_SPREAD_ENTRY_WORDS && sizeof(SpreadSummary) == 8 * SIM_SPREAD_SUMMARY_WORDS,
                "an entry's record is eight words, its summary forty");
  static_assert(sizeof(LedgerSample::Entry) == 8 * SIM_LEDGER_ENTRY_WORDS, "an entry's record is eight words");
  static_assert(sizeof(TrafficSample) == 8 * SIM_TRAFFIC_WORDS && sizeof(TrafficSummary) == 8 * SIM_TRAFFIC_SUMMARY_WORDS,
                "a traffic sample is sixty-four words, a column's summary forty");
  std::vector<sim_gazette_row> gazette_rows(int (*rows)(sim_handle*, uint32_t, uint32_t, sim_gazette_row*), const char* what, uint32_t first, uint32_t n) {
    if (n == 0xFFFFFFFFu) n = n_ > first ? n_ - first : 0;
    std::vector<sim_gazette_row> out(n ? n : 1);
    check(rows(h_, first, n, out.data()), what);
    out.resize(n);
    return out;
  }
  static_assert(sizeof(GazetteSample) == 8 * SIM_GAZETTE_WORDS, "a gazette sample is sixty-four words");
  // what the periodic observers share: the count, and "read n samples of `stride` words and unpack each"
  std::pair<uint32_t, uint32_t> sample_count(int (*count)(const sim_handle*, uint32_t*, uint32_t*), const char* what) const {
    uint32_t t = 0, d = 0;
    check(count(h_, &t, &d), what);
    return {t, d};
  }
  template <typename Sample, typename Unpack>
  std::vector<Sample> sample_read(int (*count)(const sim_handle*, uint32_t*, uint32_t*),
                                  int (*read)(sim_handle*, uint32_t, uint32_t, uint64_t*, size_t, uint32_t*), const std::string& group,
                                  uint32_t first, uint32_t n, size_t stride, Unpack unpack_one) {
    if (n == 0xFFFFFFFFu) { const uint32_t t = sample_count(count, (group + "_count").c_str()).first; n = t > first ? t - first : 0; }
    std::vector<uint64_t> words((n ? n : 1) * stride);
    uint32_t got = 0;
    check(read(h_, first, n, words.data(), words.size(), &got), (group + "_read").c_str());
    std::vector<Sample> out(got);
    for (uint32_t i = 0; i < got; ++i) unpack_one(words.data() + i * stride, out[i]);
    return out;
  }
  // a sample's words -> its header (the first sizeof(Header) bytes) and the n records behind it
  template <typename Header, typename Rec>
  static void unpack(const uint64_t* w, size_t n, Header& header, std::vector<Rec>& recs) {
    std::memcpy(&header, w, sizeof header);
    recs.resize(n);
    if (n) std::memcpy(recs.data(), w + sizeof header / 8, n * sizeof(Rec));
  }
};

inline std::vector<Member> Serf::members() const {
  std::vector<uint8_t> st(c_->size());
  std::vector<uint64_t> lt(c_->size());
  check(sim_members(c_->raw(), id_, st.data(), lt.data(), c_->size()), "sim_members");
  std::vector<Member> out;
  for (uint32_t i = 0; i < c_->size(); ++i)
    if (st[i] != 0) out.push_back(Member{i, (MemberStatus)st[i], lt[i]});
  return out;
}
inline Stats Serf::stats() const {
  Stats s;
  check(sim_stats_get(c_->raw(), id_, &s), "sim_stats_get");
  return s;
}
inline void Serf::user_event(uint32_t key, uint32_t len, bool cc) { check(sim_user_event(c_->raw(), id_, key, len, cc), "sim_user_event"); }
inline void Serf::user_event(const std::string& name, const std::vector<uint8_t>& payload, bool cc, size_t max_user_event_size) {
  constexpr size_t USER_EVENT_SIZE_LIMIT = 9 * 1024;  // serf.rs:44
  size_t before = name.size() + payload.size();
  if (before > max_user_event_size) throw Error(SIM_ETOOBIG, "user event exceeds configured limit before encoding");
  if (before > USER_EVENT_SIZE_LIMIT) throw Error(SIM_ETOOBIG, "user event exceeds sane limit before encoding");
  wire::Bytes nm(name.begin(), name.end());
  size_t len = wire::user_event_len(stats().event_time, nm, payload, cc);
  if (len > max_user_event_size || len > USER_EVENT_SIZE_LIMIT) throw Error(SIM_ETOOBIG, "encoded user event exceeds limit");
  user_event(wire::event_key(nm, payload), (uint32_t)len, cc);
}
inline void Serf::query(uint32_t qid, uint32_t flags) { check(sim_query(c_->raw(), id_, qid, flags), "sim_query"); }
inline void Serf::query(uint32_t qid, uint32_t flags, const std::vector<uint32_t>& ids, uint32_t tag_mask) {
  check(sim_query_filtered(c_->raw(), id_, qid, flags, ids.data(), (uint32_t)ids.size(), tag_mask), "sim_query_filtered");
}
inline void Serf::set_tags(uint32_t tag_class) { check(sim_set_tags(c_->raw(), id_, tag_class), "sim_set_tags"); }
inline Serf::QueryStatus Serf::query_status(uint32_t qid) const {
  QueryStatus st{0, 0, false};
  int open = 0;
  check(sim_query_status(c_->raw(), qid, &st.acks, &st.responses, &open), "sim_query_status");
  st.open = open != 0;
  return st;
}
// (SIM_EINVAL from the two tracker reads means "this id does not own its tracker entry": before the tick that executes the
// query has run — the channels exist and are empty, query.rs:201-212 — or after a newer query with the same residue took the
// entry over — the reference's receivers would simply be closed.  Neither is an error of the caller.)
inline bool Serf::QueryResponse::finished() const {
  if (closed_) return true;
  uint64_t a, r;
  int open = 0;
  const int rc = sim_query_status(c_->raw(), id_, &a, &r, &open);
  // not started yet: still open; evicted: finished — and an id that never gets to own its tracker entry (taken over by a newer query
  // of the same residue before this object ever saw it; an id that was never valid) is finished once its deadline is past, so that
  // `while (!r.finished()) step()` ends
  if (rc == SIM_EINVAL) return started_ || c_->tick() > give_up_;
  check(rc, "sim_query_status");
  started_ = true;
  return !open;
}
inline Serf::QueryResponse::QueryResponse(Cluster* c, uint32_t id) : c_(c), id_(id) {
  uint32_t n = c->size(), digits = 0;
  while (n) { ++digits; n /= 10; }
  give_up_ = c->tick() + 2u + 16u * digits;
}
inline std::vector<uint32_t> Serf::QueryResponse::fresh(int which, std::vector<uint32_t>& seen) {
  std::vector<uint32_t> out;
  if (closed_) return out;
  uint32_t n = 0;
  const int rc = sim_query_responders(c_->raw(), id_, which, nullptr, 0, &n);
  if (rc == SIM_EINVAL) return out;  // nobody yet (the query's tick has not run) or nobody any more (tracker taken over)
  check(rc, "sim_query_responders");
  started_ = true;
  std::vector<uint32_t> all(n);
  if (n) check(sim_query_responders(c_->raw(), id_, which, all.data(), n, &n), "sim_query_responders");
  std::set_difference(all.begin(), all.end(), seen.begin(), seen.end(), std::back_inserter(out));  // both ascending
  seen = std::move(all);
  return out;
}
inline std::vector<uint32_t> Serf::QueryResponse::acks() { return fresh(0, seen_acks_); }
inline std::vector<Serf::NodeResponse> Serf::QueryResponse::responses() {
  std::vector<NodeResponse> out;
  for (uint32_t from : fresh(1, seen_resp_)) out.push_back(NodeResponse{from, payload_of_ ? payload_of_(from) : std::vector<uint8_t>{}});
  return out;
}
inline void Serf::join(uint32_t peer) { check(sim_join(c_->raw(), id_, peer), "sim_join"); }
inline void Serf::leave() { check(sim_leave(c_->raw(), id_), "sim_leave"); }
inline void Serf::shutdown() { check(sim_inject(c_->raw(), c_->tick(), SIM_OP_CRASH, id_, 0, 0), "sim_inject"); }
inline void Serf::remove_failed_node(uint32_t id) { check(sim_force_leave(c_->raw(), id_, id, 0), "sim_force_leave"); }
inline void Serf::remove_failed_node_prune(uint32_t id) { check(sim_force_leave(c_->raw(), id_, id, 1), "sim_force_leave"); }
inline void Serf::subscribe() { check(sim_watch(c_->raw(), id_), "sim_watch"); }

}  // namespace serf
