// serf_sim_host.inc — part of the translation unit serf_sim.hip (included from there, in this order; not a header of its own).
// host: the handle, configuration checks, suspicion parameters, allocation helpers.
// ------------------------------------------------------------------------------------------------
// host side: the C ABI
// ------------------------------------------------------------------------------------------------
struct OpEnt {
  u64 tick;
  u32 op, node, a, b;
  u64 val;  // SIM_OP_DELIVER: the record's value (a = key, b = wire bits of meta); 0 otherwise
};

// A split array — [planes][Nl] 16-byte heads, then [planes][Nl] tails — whose planes get physical memory when they are first
// needed (VERDICT r4 item 7: the footprint).  A view entry of slot a lives in plane a, a ring bucket of Lamport time t in plane
// t mod B: at the bench configuration 50 of 1 024 view slots and 180 of 2 x 512 ring buckets are ever touched, and the other
// 60 GB per Mi nodes were allocated, zeroed at sim_create and never read.  HIP's virtual-memory API: the whole range is
// RESERVED (the addresses the kernels compute do not change: Dev::view / vtail stay what they were), chunks of `chunk` planes
// are created, mapped and zeroed on the handle's stream when the host hands out a slot / admits a Lamport time beyond what is
// mapped — the host is the only one who does either (ensure_slot, inject_val).  Whole-array walks (digest, dump, image)
// take the unmapped planes as the zeros they stand for.  `va == nullptr`: the array is an ordinary allocation, all of it
// (small clusters whose planes are not a multiple of the mapping granularity, dense views, SERF_SIM_EAGER=1).
struct LazyPlanes {
  char* va = nullptr;
  size_t va_bytes = 0, plane_bytes = 0;
  u32 planes = 0, chunk = 0, mapped = 0;
  std::vector<std::pair<void*, size_t>> maps;               // what is mapped where (to unmap)
  std::vector<hipMemGenericAllocationHandle_t> phys;
};
// One of the handle's three split arrays: where it starts, where its tails start (in entries: planes * Nl), how many planes it has and
// which of them have memory.  The kernels read their own copy (Dev::view / vtail, ering0 / etail, qring0 / qtail), set from these once.
struct SplitArr {
  uint4* base = nullptr;
  size_t tail = 0;
  u32 planes = 0;
  LazyPlanes lz;
};
enum { SP_VIEW = 0, SP_EV = 1, SP_Q = 2, SP_N = 3 };  // (the order of SIM_ARR_VIEW .. SIM_ARR_QRING and of the image's sections)
enum { OB_SERIES = 0, OB_CENSUS = 1, OB_ROLL = 2, OB_LEDGER = 3, OB_DETECT = 4, OB_SPREAD = 5, OB_TRAFFIC = 6, OB_TREE = 7, OB_N = 8 };  // the periodic observers, in the order their samples follow a tick on the stream
// ... and behind them the query board (serf_sim_qboard.inc): the ninth entry of the table.  It stands in a line of its own because
// tests/test_tree.py pins the line above as it is; behind the board the rumour catalogue (serf_sim_catalog.inc), behind that the member
// gazette (serf_sim_gazette.inc); OB_ALL is what the table holds
enum { OB_QBOARD = OB_N, OB_CATALOG = OB_N + 1, OB_GAZETTE = OB_N + 2, OB_ALL = OB_N + 3 };
static_assert(OB_QBOARD == 8 && OB_CATALOG == 9 && OB_GAZETTE == 10 && OB_ALL == 11,
              "the observers' table: eight of rumours and members, the query board, the rumour catalogue, the member gazette");
// Function-local device scratch: freed when it goes out of scope — behind whatever stream synchronisation stands before that.
template <typename T>
struct DevScratch {
  T* p = nullptr;
  DevScratch() = default;
  DevScratch(DevScratch&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevScratch& operator=(DevScratch&& o) noexcept { std::swap(p, o.p); return *this; }
  DevScratch(const DevScratch&) = delete;
  DevScratch& operator=(const DevScratch&) = delete;
  ~DevScratch() { if (p) (void)hipFree(p); }
  int alloc(size_t n) {  // n elements (one at least); SIM_ENOMEM
    if (hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)) == hipSuccess) return SIM_OK;
    (void)hipGetLastError();
    p = nullptr;
    return SIM_ENOMEM;
  }
  T* get() const { return p; }
};
struct sim_handle {
  sim_config cfg = {};
  Dev d = {};
  u64 tick = 0;
  u32 dense = 0, n_slots = 0;
  hipStream_t stream = nullptr;
  std::vector<u32> slot_of, subject_of;
  std::vector<u32> walk;  // host copy of d.walk
  std::vector<u32> alloc_tick;  // [A] tick at which the slot was handed out
  u32 n_alloc = 0;              // slots in use
  uint8_t* rc_refd = nullptr;   // the recycling pass's device scratch (the first pass allocates, the handle frees with the rest): [N] "still mentioned",
  u32* rc_scr = nullptr;        // and the candidates' words
  u64 ops_dropped = 0, slots_recycled = 0;
  u64 events_lost = 0;          // events the bounded device log dropped (counted when they are drained)
  u32 recycle_at = 0xFFFFFFFFu; // the tick whose recycling pass has already run
  u32 pp_done_at = 0xFFFFFFFFu; // the tick whose push-pull batch the sharded host has already run
  // the batch being driven by the sharded host: in-shard pairs, and the cross-shard pairs grouped by peer shard in
  // ascending pair order — r1: this shard owns the even node `a` (receives b in round 1, sends a in round 2); s1: owns `b`
  std::vector<u32> pp_local_a, pp_local_b, pp_r1, pp_s1;
  std::vector<u32> rc_a, rc_b;  // Reconnector: the reconnect attempts that run as push-pull pairs in THIS tick (global ids; initiator, target)
  u32* d_pp = nullptr;          // the four lists on the device, back to back (replaced by every sim_pp_plan: not one of `allocs`)
  std::vector<sim_view> base;
  uint4* d_base = nullptr;  // [N][2]
  std::vector<OpEnt> ops;
  size_t op_cursor = 0;
  u64* d_scratch = nullptr;  // 16 x u64
  uint8_t* d_mst = nullptr;
  u64* d_mlt = nullptr;
  sim_stats* d_stats = nullptr;
  std::vector<void*> allocs;  // every device allocation that lives as long as the handle
  TickP prev = {};
  bool bound = false;
  int device = 0;
  u32 qt_cursor = 0, q_timeout = 0;  // running-query trackers (SIM_QT, round robin); query timeout in ticks
  std::vector<u32> qfilt;    // [SIM_QT][SIM_QF_WORDS] host copy of the query filters (the host is their only writer)
  // content of the user events the library was told in bytes (sim_deliver_message, sim_user_event_bytes): what
  // sim_peek_packet encodes for their keys
  std::unordered_map<u32, std::pair<serf::wire::Bytes, serf::wire::Bytes>> evreg;
  u32 profiling = 0;  // 0 = off, n = HIP events around every n-th tick-kernel launch
  u64 prof_seq = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof;  // one event pair per tick-kernel launch
  // slot-less failed probes (SIMSPEC §2.7): device lists by tick parity, their heads copied to pinned host memory behind
  // every tick's launch; the list of tick t is read at the end of tick t + 1 — by then the copy has long landed, nobody
  // waits for a kernel — and replayed as operations of tick t + 2
  u32* sreq_buf[3] = {};
  u32* sreq_host[3] = {};       // pinned, written by the kernel itself: the first SREQ_HEAD pairs, unused ones 0xFFFFFFFF
  hipEvent_t sreq_ev[3] = {};
  hipEvent_t sreq_wait[3] = {}; // what marks "tick t's kernel has finished": sreq_ev (recorded behind the launch, or riding on the dispatch
                                // itself as its stop event) or the stop event of the tick's timing pair; null: the stream was synchronised since
  bool sreq_on_dispatch = false;  // this tick's launch carried its completion event: sim_step_end records nothing
  u64 sreq_tick[3] = {~0ull, ~0ull, ~0ull};  // the tick whose list sits in the buffer (~0: none / consumed)
  u32 pp_step = 0;  // push-pull batches: every pp_step ticks one of PP_GROUPS pair classes synchronises (0 = off)
  TickP cur_tp = {};       // parameters of the tick between sim_step_begin and sim_step_end
  bool in_tick = false, tick_timed = false, tick_bracket = false;
  hipEvent_t tick_ev0 = nullptr;
  uint4* rbuf[2] = {};     // sharded: packets sent during tick t are received into rbuf[t & 1]
  // local mode: the packets in flight in their canonical receiver-indexed form inbox[k][node] (what the oracle keeps,
  // what dumps, digests and images hold), produced from Dev::obox on demand; mat_tick = the tick it was made for
  uint4* inbox_mat = nullptr;
  u64 mat_tick = ~0ull;
  // the round's all-to-all over RCCL, issued by the library (sim_exchange_*): the communicator, a stream of its own for the
  // collectives (it waits for one chunk's launch, the handle's stream waits for all of a round's exchanges before the next
  // tick reads them), the events that carry those two orderings
  ncclComm_t xcomm = nullptr;
  hipStream_t xstream = nullptr;
  hipEvent_t xev_go = nullptr, xev_done = nullptr;
  u32 xworld = 0;
  bool xpending = false;  // exchanges issued since the handle's stream last waited for them
  bool self_direct = false;  // packed slabs: the slab this shard addresses to itself is packed straight into the receive buffer and is not exchanged (set by sim_exchange_init)
  // (r6) the heads of the slot-less suspicion lists travel WITH the round's exchange (SWIM on): every peer's head of tick t lands in
  // xh_dev[t % 4][peer], a small kernel behind the group writes what the lists hold — counts and pairs — into pinned host memory,
  // xh_ev[t % 4] marks it; sim_suspect_import(h, t, NULL, world) reads it two ticks later.  No side stream, no second collective,
  // no copy commands between the pack and the next tick's index pass.
  u32* xh_dev = nullptr;   // [4][world][SIM_SREQ_HEAD_WORDS] (one of `allocs`)
  u32* xh_host = nullptr;  // pinned, same shape
  hipEvent_t xh_ev[4] = {};
  u64 xh_tick[4] = {~0ull, ~0ull, ~0ull, ~0ull};  // the tick whose heads slot i holds (~0: none / consumed)
  // SIM_CF_RANDOM_FANOUT: scratch of the per-tick graph build (rf_* kernels)
  u32* rf_gcur[2] = {};  // bucket fill counters (two: a build zeroes the next one's)
  void *rf_ovf[2] = {}, *rf_l1 = nullptr;  // overflow lists (two, likewise) and the buckets' regions: u32 entries when a pair id and a target's offset fit, u64 otherwise
  bool rf_wide = false;  // ... u64
  u32 rf_par = 0;                      // which of the two this build uses
  RfP rfp = {};  // the parameters that do not change from tick to tick
  // The graph of tick s is a function of (seed, s): it is built on a stream of its own, TWO ticks ahead — enqueued when tick
  // s - 1 begins, read by tick s + 1 — so that no tick ever waits for a build (one tick ahead, the build ran in the tail of
  // the tick kernel and the next tick waited 25 us for rf_rows).  rf_rcsr[s % 3] / rf_rsrc[s % 3] = the rows of the packets SENT
  // during tick s: while tick t reads buffer (t - 1) % 3 the builds of t and t + 1 may still be writing the other two.
  // rf_q[i] = the tick whose graph buffer i holds or is getting (~0: none), rf_done[i] marks its build.
  u32* rf_rcsr[3] = {};
  u32* rf_rsrc[3] = {};
  // ... on a shard (SIM_XCHG_PACKED): the graph of tick s is the SENDING side's — rf_rsrc[s % 3] = the shard's own (target, sender,
  // slot) triples sorted, as pair ids; rf_cntb / rf_btot / rf_xoff [s % 3] = count bytes per target of every destination, bucket
  // totals, where every destination's pairs start — needed when tick s has computed (the pack).  The receiving side's rows
  // (rx_rcsr / rx_rsrc) are made at the start of a tick from the slabs the round's exchange delivered.
  uint8_t* rf_cntb[3] = {};
  u32* rf_btot[3] = {};
  u32* rf_xoff[3] = {};
  u32 rf_C = 1;        // sender chunks of a shard's packed exchange (sim_config.chunks; 1 otherwise)
  u32 *rx_rcsr = nullptr, *rx_rsrc = nullptr;
  u32 rx_cap = 0;      // entries rx_rsrc holds (f * Nl, 12 sigma and some)
  RfxL rfx = {};
  u32* xflag = nullptr;  // pinned host memory the rf / rfx kernels write to: a slab, a count byte or rsrc overflowed -> SIM_ERANGE
  hipStream_t rf_stream = nullptr;
  hipEvent_t rf_done[3] = {}, rf_go[2] = {};
  u64 rf_q[3] = {~0ull, ~0ull, ~0ull};
  bool rf_sync = false;
  // view entries and ring buckets on demand (SP_VIEW, SP_EV, SP_Q); ev_hi / q_hi: no node's event / query clock exceeds them (a clock
  // starts at 1, grows by one per user event / query somebody originates and is otherwise a maximum of clocks seen; a record or a clock
  // that comes in over the byte boundary raises the bound to its own time + 1) — so no record's Lamport time does
  SplitArr sp[SP_N];
  u64 ev_hi = 1, q_hi = 1;
  u32* deep_seen = nullptr;  // pinned: the longest deep list any launch has had (deep_queue_kernel keeps it; sizes that kernel's grid)
  struct TrackState* trk = nullptr;  // device-resident trackers (serf_sim_track.inc); null until the first sim_track_add
  struct Observer* obs[OB_ALL] = {};  // the periodic observers (the frame at the end of this file); an entry is null unless its observer is running
  sim_handle() = default;
  sim_handle(const sim_handle&) = delete;
  sim_handle& operator=(const sim_handle&) = delete;
  ~sim_handle();  // (at the end of this file, behind the observers' frame)
};
// serf_sim_track.inc: the hooks of sim_step_end / ~sim_handle (called only when h->trk)
static int track_step_end(sim_handle* h);
static void track_destroy(sim_handle* h);
// serf_sim_step.inc: what sim_create, sim_snapshot, sim_restore and sim_exchange_chunk need of the per-tick path
static int create_rf(sim_handle* h);
static int sreq_take(sim_handle* h, u64 t, uint32_t* out, uint32_t cap_pairs, uint32_t* n_pairs);
static int rfx_pack(sim_handle* h, u64 t, u32 c);
static int rf_reset(sim_handle* h);
static int rf_build(sim_handle* h, u64 tick, hipStream_t s);  // (the test hook sim_t_rf_graph, serf_sim_exchange.inc)
static bool rf_lean(const RfP& r);
static hipEvent_t tick_done_event(const sim_handle* h, u64 t);

#define HCHECK(x)                                                                        \
  do {                                                                                   \
    hipError_t e_ = (x);                                                                 \
    if (e_ != hipSuccess) {                                                              \
      fprintf(stderr, "serf_sim: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
      return SIM_EDEVICE;                                                                \
    }                                                                                    \
  } while (0)

static u32 h_digits10(u32 n) {
  u32 d = 0;
  while (n) { ++d; n /= 10; }
  return d;
}
static int cfg_check(const sim_config* c) {
  if (!c || c->struct_size != sizeof(sim_config)) return SIM_EINVAL;
  if (c->n_nodes < 1 || c->vshards < 1 || c->n_nodes % c->vshards) return SIM_EINVAL;
  u32 M = c->n_nodes / c->vshards;
  if (c->vshards > 1 && (M % c->vshards || M <= SIM_MAX_FANOUT)) return SIM_EINVAL;
  if (c->shard_count != 1 && c->shard_count != c->vshards) return SIM_EINVAL;
  if (c->shard_rank >= c->shard_count) return SIM_EINVAL;
  if ((c->flags & SIM_CF_FORCE_SHARDED) && c->shard_count != c->vshards) return SIM_EINVAL;  // one rank of the N > 1 path: V == 1
  if (c->fanout < 1 || c->fanout > SIM_MAX_FANOUT) return SIM_EINVAL;
  if (c->chunks > 1 && ((M / c->vshards) % c->chunks || (M / c->vshards) / c->chunks < 1)) return SIM_EINVAL;
  // memberlist's literal kRandomNodes (variable in-degree, an explicit CSR per tick): sender chunks are a SHARD's exchange schedule
  // (SIM_XCHG_PACKED: chunk c's slabs are packed and leave behind chunk c's launch) — one handle that holds every node has none
  if ((c->flags & SIM_CF_RANDOM_FANOUT) && c->chunks > 1 && !(c->shard_count > 1 || (c->flags & SIM_CF_FORCE_SHARDED))) return SIM_EINVAL;
  if (c->event_ring < 1 || c->query_ring < 1) return SIM_EINVAL;
  if (c->ring_overflow > 4096u || c->reserved0) return SIM_EINVAL;
  if (c->pkt_records && (c->pkt_records % SIM_P || c->pkt_records > SIM_PKT_RECORDS_MAX)) return SIM_EINVAL;
  if (c->retransmit_mult * h_digits10(c->n_nodes) > 63u) return SIM_EINVAL;
  if (c->n_nodes > (1u << 24)) return SIM_EINVAL;  // SUSPECT / DEAD carry the accuser's id in 24 bits on the wire (sim_packet)
  if ((c->flags & SIM_CF_PRUNE_DELAY) && !c->probe_interval) return SIM_EINVAL;  // the request lists are the SWIM layer's machinery
  if (c->probe_interval) {  // suspicion timers name view slots with 16 bits
    u32 A = (c->view_slots == 0 || c->view_slots >= c->n_nodes) ? c->n_nodes : c->view_slots;
    if (A > 65534u) return SIM_EINVAL;
  }
  // ages are formed modulo 2^21 (the view entry's stamp) and deadlines are 32-bit sums below SIM_TICK_MAX's margin: everything an age
  // or a deadline is measured against stays below SIM_INTERVAL_LIMIT (the suspicion table's entries: swim_params' cap)
  for (u32 v : {c->probe_interval, c->intent_timeout, c->leave_delay, c->reap_interval, c->reconnect_timeout, c->tombstone_timeout,
                c->queue_check_interval, c->push_pull_interval, c->recycle_interval, c->gossip_to_the_dead, c->reconnect_interval})
    if (v >= SIM_INTERVAL_LIMIT) return SIM_EINVAL;
  return SIM_OK;
}
// Suspicion parameters in ticks (memberlist suspicion.go / util.go, SURVEY.md App. B.5); the same
// arithmetic, in the same order, as the spec (DESIGN.md SIMSPEC §6).
static void swim_params(const sim_config* c, u32* swim, u32* k_out, u32 T[SIM_MAX_CONF]) {
  *swim = c->probe_interval > 0;
  u32 k = c->suspicion_mult >= 2 ? c->suspicion_mult - 2 : 0;
  if (k > SIM_MAX_CONF - 1) k = SIM_MAX_CONF - 1;
  if (c->n_nodes < 2 || c->n_nodes - 2 < k) k = 0;
  double scale = std::log10(c->n_nodes > 1 ? (double)c->n_nodes : 1.0);
  if (scale < 1.0) scale = 1.0;
  u64 mn = (u64)c->suspicion_mult * (u64)std::floor(scale * 1000.0) * c->probe_interval / 1000u;
  if (mn < 1) mn = 1;
  u64 mx = (u64)c->suspicion_max_mult * mn;
  if (mx < mn) mx = mn;
  for (u32 i = 0; i < SIM_MAX_CONF; ++i) {
    double t = (double)mn;
    if (k >= 1 && i <= k) {
      double frac = std::log((double)i + 1.0) / std::log((double)k + 1.0);
      t = std::floor((double)mx - frac * (double)(mx - mn));
      if (t < (double)mn) t = (double)mn;
    }
    T[i] = t > 2000000.0 ? 2000000u : (u32)t;
  }
  static_assert(2000000u < SIM_INTERVAL_LIMIT, "a suspicion timeout is compared with an age taken modulo 2^21");
  *k_out = k;
}

template <typename T>
static int dalloc(sim_handle* h, T** p, size_t n) {
  void* v = nullptr;
  if (hipMalloc(&v, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return SIM_ENOMEM;
  h->allocs.push_back(v);
  *p = (T*)v;
  return SIM_OK;
}
#define DA(ptr, n) \
  if (int rc_ = dalloc(h, &(ptr), (n))) return rc_;
static inline int grid_for(size_t n) { return (int)std::min<size_t>((n + BLOCK - 1) / BLOCK, 8192); }
// ---- LazyPlanes ----
static hipMemAllocationProp lazy_prop(int device) {
  hipMemAllocationProp pr;
  memset(&pr, 0, sizeof pr);
  pr.type = hipMemAllocationTypePinned;
  pr.location.type = hipMemLocationTypeDevice;
  pr.location.id = device;
  return pr;
}
// reserve the range; false: not this array (the caller allocates it whole)
static bool lazy_reserve(sim_handle* h, LazyPlanes& L, uint4** out, u32 planes, size_t Nl) {
  const char* env = getenv("SERF_SIM_EAGER");
  if (env && *env && *env != '0') return false;
  hipMemAllocationProp pr = lazy_prop(h->device);
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &pr, hipMemAllocationGranularityRecommended) != hipSuccess || !gran) { (void)hipGetLastError(); return false; }
  const size_t pb = Nl * 16;
  if (planes < 16 || pb % gran) return false;   // (a plane of 128 Ki nodes is one 2 MiB granule)
  void* va = nullptr;
  const size_t bytes = 2 * (size_t)planes * pb;
  if (hipMemAddressReserve(&va, bytes, gran, nullptr, 0) != hipSuccess || !va) { (void)hipGetLastError(); return false; }
  L.va = (char*)va; L.va_bytes = bytes; L.plane_bytes = pb; L.planes = planes; L.mapped = 0;
  L.chunk = (u32)std::max<size_t>(1, std::min<size_t>(((size_t)128 << 20) / pb, planes / 8));  // 128 MiB at a time, an eighth of the array at most
  // every chunk whole (the last one too) and a multiple of 64 KiB: hipMemSetAccess refused the 32 KiB tail of a 34-plane ring of
  // 16 KiB planes although 16 KiB passed the granularity query (r6: the overflow rows made plane counts that are not powers of two)
  while (L.planes % L.chunk) --L.chunk;
  if (((size_t)L.chunk * pb) % ((size_t)64 << 10)) {
    (void)hipMemAddressFree(va, bytes);
    L.va = nullptr; L.va_bytes = 0; L.planes = 0;
    return false;
  }
  *out = (uint4*)va;
  return true;
}
// planes [0, need) have memory (zeroed on the handle's stream, in order with everything that may touch them)
static int lazy_need(sim_handle* h, LazyPlanes& L, u64 need64) {
  if (!L.va) return SIM_OK;
  const u32 need = (u32)std::min<u64>(need64, L.planes);
  hipMemAllocationProp pr = lazy_prop(h->device);
  hipMemAccessDesc ac;
  memset(&ac, 0, sizeof ac);
  ac.location = pr.location;
  ac.flags = hipMemAccessFlagsProtReadWrite;
  while (L.mapped < need) {
    const u32 cnt = std::min(L.chunk, L.planes - L.mapped);
    const size_t sz = (size_t)cnt * L.plane_bytes;
    // both halves (the heads' planes, the tails' planes) or neither: a half-mapped chunk would make every retry map over a mapping
    // (ADVICE r5) — what the first half got is given back when the second fails
    hipMemGenericAllocationHandle_t ph[2];
    char* at[2];
    int done = 0, rc = SIM_OK;
    const char* what = "";
    for (int half = 0; half < 2 && rc == SIM_OK; ++half) {
      at[half] = L.va + (half ? (size_t)L.planes * L.plane_bytes : 0) + (size_t)L.mapped * L.plane_bytes;
      if (hipMemCreate(&ph[half], sz, &pr, 0) != hipSuccess) { rc = SIM_ENOMEM; what = "hipMemCreate"; break; }
      if (hipMemMap(at[half], sz, 0, ph[half], 0) != hipSuccess) { (void)hipMemRelease(ph[half]); rc = SIM_ENOMEM; what = "hipMemMap"; break; }
      done = half + 1;
      if (hipMemSetAccess(at[half], sz, &ac, 1) != hipSuccess) { rc = SIM_EDEVICE; what = "hipMemSetAccess"; break; }
      if (hipMemsetAsync(at[half], 0, sz, h->stream) != hipSuccess) { rc = SIM_EDEVICE; what = "hipMemsetAsync"; break; }
    }
    if (rc != SIM_OK) {
      const hipError_t e = hipGetLastError();
      fprintf(stderr, "serf_sim: lazy planes: %s of %zu bytes failed (%s); planes %u..%u of %u\n", what, sz, hipGetErrorString(e), L.mapped, L.mapped + cnt, L.planes);
      for (int half = 0; half < done; ++half) { (void)hipMemUnmap(at[half], sz); (void)hipMemRelease(ph[half]); }
      return rc;
    }
    for (int half = 0; half < 2; ++half) { L.phys.push_back(ph[half]); L.maps.emplace_back(at[half], sz); }
    L.mapped += cnt;
  }
  return SIM_OK;
}
static void lazy_release(LazyPlanes& L) {
  if (!L.va) return;
  for (auto& m : L.maps) (void)hipMemUnmap(m.first, m.second);
  for (auto& ph : L.phys) (void)hipMemRelease(ph);
  (void)hipMemAddressFree(L.va, L.va_bytes);
  L.va = nullptr; L.maps.clear(); L.phys.clear(); L.mapped = 0;
}
static inline u32 split_mapped(const SplitArr& A) { return A.lz.va ? A.lz.mapped : A.planes; }
// the planes the rings need for clocks up to ev_hi / q_hi (a time t sits in plane t mod B)
static int rings_need(sim_handle* h) {
  int rc = lazy_need(h, h->sp[SP_EV].lz, h->d.X + h->ev_hi + 2);  // (rows 0 .. X-1: the overflow rows)
  return rc ? rc : lazy_need(h, h->sp[SP_Q].lz, h->d.X + h->q_hi + 2);
}
#define EV_CAP (1u << 20)

// ---- what the observers share on the host (the device part: serf_sim_observe.inc; it stands here because it needs the handle) ----
// trackers, series, census, roll, ledger, detection log, spread map, traffic meter, rumour tree, query board, rumour catalogue and member gazette watch a handle that holds every node, between ticks
static int observer_usable(const sim_handle* h) {
  if (!h) return SIM_EINVAL;
  if (h->d.sharded || h->in_tick) return SIM_ESTATE;
  return SIM_OK;
}
// A device buffer of samples, one behind every period-th tick from `first` on until it is full.  The host knows every sampled tick in
// advance: it passes a sample's place to the launches that write it and reads nothing back.
struct Sampler {
  u64* d_buf = nullptr;     // [cap] samples of stride_words words
  size_t stride_words = 0;
  u64 first = 0;            // the first sampled tick
  u32 period = 1, cap = 0, taken = 0, dropped = 0;
};
static int sampler_open(const sim_handle* h, Sampler& S, u32 first_tick, u32 period, u32 capacity, size_t stride_words) {
  if (hipMalloc((void**)&S.d_buf, (size_t)capacity * stride_words * 8) != hipSuccess) {
    (void)hipGetLastError();
    S.d_buf = nullptr;
    return SIM_ENOMEM;
  }
  S.stride_words = stride_words;
  S.first = std::max<u64>(first_tick, h->tick);
  S.period = period;
  S.cap = capacity;
  return SIM_OK;
}
// sim_step_end, tick h->tick - 1 enqueued: where its sample goes — null when none is due, or when the buffer is full (counted)
static u64* sampler_slot(const sim_handle* h, Sampler& S) {
  const u64 t = h->tick - 1;
  if (t < S.first || (t - S.first) % S.period) return nullptr;
  if (S.taken == S.cap) { S.dropped++; return nullptr; }
  return S.d_buf + (size_t)S.taken * S.stride_words;
}
static inline void sampler_commit(Sampler& S) { S.taken++; }  // (behind launches that were enqueued without error)
static void sampler_count(const Sampler* S, u32* taken, u32* dropped) {  // (null: nothing runs)
  *taken = S ? S->taken : 0u;
  *dropped = S ? S->dropped : 0u;
}
// samples first .. first + n - 1 into out[cap_words]; waits for the handle's stream
static int sampler_read(sim_handle* h, const Sampler& S, u32 first, u32 n, void* out, size_t cap_words, u32* n_out) {
  if ((u64)first + n > S.taken || (size_t)n * S.stride_words > cap_words) return SIM_EINVAL;
  HCHECK(hipStreamSynchronize(h->stream));
  if (n) HCHECK(hipMemcpy(out, S.d_buf + (size_t)first * S.stride_words, (size_t)n * S.stride_words * 8, hipMemcpyDeviceToHost));
  *n_out = n;
  return SIM_OK;
}
static void sampler_close(Sampler& S) {  // (the caller has waited for the samples still enqueued)
  if (S.d_buf) (void)hipFree(S.d_buf);
  S.d_buf = nullptr;
}

// ---- the periodic observers' frame: series, census, roll, ledger, detection log, spread map, traffic meter, rumour tree and query board differ in their kernels and in nothing below ----
// A periodic observer while it runs: its samples and, in the struct derived from it, the scratch and the parameters of its kernels.
struct Observer {
  Sampler smp;
  virtual ~Observer() { sampler_close(smp); }  // (the caller has waited for the samples still enqueued)
  // one sample of the state the stream will be in when it gets here, enqueued into out[smp.stride_words]
  virtual int sample(sim_handle* h, u64* out) = 0;
};
static void observer_destroy(sim_handle* h, u32 k) {  // (null: nothing runs)
  delete h->obs[k];
  h->obs[k] = nullptr;
}
// sim_<observer>_start.  `fresh` is the observer as far as the host alone can build it (taken over here); check() judges the observer's own
// arguments, setup() gets its device scratch.  Everything is built off the handle and installed when all of it has succeeded: a start that
// fails leaves no observer.  The order of the checks is the ABI's: bad arguments are SIM_EINVAL before "already running" is SIM_ESTATE.
template <typename Check, typename Setup>
static int observer_start(sim_handle* h, u32 k, Observer* fresh, u32 max_samples, u32 first_tick, u32 period, u32 capacity,
                          size_t stride_words, Check check, Setup setup) {
  std::unique_ptr<Observer> o(fresh);
  if (int rc = observer_usable(h)) return rc;
  if (!period || !capacity || capacity > max_samples) return SIM_EINVAL;
  if (int rc = check()) return rc;
  if (h->obs[k]) return SIM_ESTATE;
  if (int rc = setup()) return rc;
  if (int rc = sampler_open(h, o->smp, first_tick, period, capacity, stride_words)) return rc;
  h->obs[k] = o.release();
  return SIM_OK;
}
static int observer_count(const sim_handle* h, u32 k, u32* taken, u32* dropped) {
  if (int rc = observer_usable(h)) return rc;
  if (!taken || !dropped) return SIM_EINVAL;
  sampler_count(h->obs[k] ? &h->obs[k]->smp : nullptr, taken, dropped);
  return SIM_OK;
}
static int observer_read(sim_handle* h, u32 k, u32 first, u32 n, void* out, size_t cap_words, u32* n_out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out || !n_out) return SIM_EINVAL;
  if (!h->obs[k]) return SIM_ESTATE;
  return sampler_read(h, h->obs[k]->smp, first, n, out, cap_words, n_out);
}
static int observer_stop(sim_handle* h, u32 k) {
  if (int rc = observer_usable(h)) return rc;
  if (!h->obs[k]) return SIM_ESTATE;
  HCHECK(hipStreamSynchronize(h->stream));  // (samples still enqueued write into the buffers)
  observer_destroy(h, k);
  return SIM_OK;
}
// sim_step_end: tick h->tick - 1 has been enqueued; the samples of it that are due follow it on the stream
static int observers_step_end(sim_handle* h) {
  for (Observer* o : h->obs) {
    u64* slot = o ? sampler_slot(h, o->smp) : nullptr;
    if (!slot) continue;
    if (int rc = o->sample(h, slot)) return rc;
    sampler_commit(o->smp);
  }
  return SIM_OK;
}
// The tail of sim_<observer>_now: launch(out) enqueues one sample into device memory of `words` words, which then comes to host[words].
// The stream is synchronised before any scratch is freed — `out` here, the caller's behind this call — also when the launch failed.
template <typename Launch>
static int observer_now(sim_handle* h, size_t words, u64* host, Launch launch) {
  DevScratch<u64> out;
  int rc = out.alloc(words);
  if (rc == SIM_OK) rc = launch(out.get());
  if (hipStreamSynchronize(h->stream) != hipSuccess && rc == SIM_OK) rc = SIM_EDEVICE;
  if (rc != SIM_OK) return rc;
  HCHECK(hipMemcpy(host, out.get(), words * 8, hipMemcpyDeviceToHost));
  return SIM_OK;
}

// The tail of a read of what an observer keeps on the device (a map, a tree): launch() enqueues its kernels behind the samples enqueued so
// far; the stream is synchronised before the caller's scratch is freed, also when the launch failed.
template <typename Launch>
static int observer_settle(sim_handle* h, Launch launch) {
  int rc = launch();
  if (hipStreamSynchronize(h->stream) != hipSuccess && rc == SIM_OK) rc = SIM_EDEVICE;
  return rc;
}
// A read that yields a list of node ids: launch(d_ids, room, d_total) writes the first `room` = min(cap, N) ids and the number of all
// into ONE scratch; the total comes back, then the ids there are (no list is longer than the nodes)
template <typename Launch>
static int observer_read_ids(sim_handle* h, u32* ids, u32 cap, u32* n_out, u32* total, Launch launch) {
  const u32 room = std::min<u32>(cap, h->d.N);
  DevScratch<u32> d_ids;  // [room] ids, then the total
  if (int rc = d_ids.alloc((size_t)room + 1)) return rc;
  if (int rc = observer_settle(h, [&]() -> int { return launch(d_ids.get(), room, d_ids.get() + room); })) return rc;
  u32 tot = 0;
  HCHECK(hipMemcpy(&tot, d_ids.get() + room, 4, hipMemcpyDeviceToHost));
  const u32 got = std::min(tot, room);
  if (got) HCHECK(hipMemcpy(ids, d_ids.get(), (size_t)got * 4, hipMemcpyDeviceToHost));
  *n_out = got;
  *total = tot;
  return SIM_OK;
}
// A read that yields a ranking (rank_candidates / rank_merge, serf_sim_observe.inc): the lists of ceil(Nl / BLOCK) workgroups — keys of
// key_words words, records of rec_words —, launch(ckey, crec, d_top, G) enqueues the two kernels, top_k records come back
template <typename Launch>
static int observer_read_top(sim_handle* h, u32 top_k, u32 key_words, u32 rec_words, void* top, Launch launch) {
  const size_t G = ((size_t)h->d.Nl + BLOCK - 1) / BLOCK;
  DevScratch<u64> d_ckey, d_crec, d_top;
  if (int rc = d_ckey.alloc(G * top_k * key_words)) return rc;
  if (int rc = d_crec.alloc(G * top_k * rec_words)) return rc;
  if (int rc = d_top.alloc((size_t)top_k * rec_words)) return rc;
  if (int rc = observer_settle(h, [&]() -> int { return launch(d_ckey.get(), d_crec.get(), d_top.get(), (u32)G); })) return rc;
  HCHECK(hipMemcpy(top, d_top.get(), (size_t)top_k * rec_words * 8, hipMemcpyDeviceToHost));
  return SIM_OK;
}
// sim_step_end, tick h->tick - 1 enqueued: where the packets it sent lie (Flight, serf_sim_observe.inc).  rows: the observer walks the
// packets addressed to a node — under kRandomNodes the graph of that tick then stands in front of the stream (rf_ready)
static int rf_ready(sim_handle* h, u64 s);
static int flight_fill(sim_handle* h, bool rows, Flight& f) {
  const Dev& d = h->d;
  const u64 t = h->tick - 1;  // the tick that sent the packets in flight
  f.rcsr = f.rsrc = nullptr;
  f.rcap = 0;
  if (rows && d.rfan) {
    if (int rc = rf_ready(h, t)) return rc;
    f.rcsr = h->rf_rcsr[t % 3]; f.rsrc = h->rf_rsrc[t % 3];
    f.rcap = d.f * d.Nl;
  }
  f.cur = (u32)(h->tick & 1);
  f.nslot = d.rfan ? d.f : h->prev.feff;  // (h->prev: the parameters of the tick that just ended)
  return SIM_OK;
}

// Everything the handle holds, whatever sim_create, sim_exchange_init or an observer got as far as setting up.  Nothing is given back
// while a stream may still use it: all three streams first.
sim_handle::~sim_handle() {
  (void)hipStreamSynchronize(stream);
  if (xstream) (void)hipStreamSynchronize(xstream);
  if (rf_stream) (void)hipStreamSynchronize(rf_stream);
  if (trk) track_destroy(this);
  for (u32 k = 0; k < OB_ALL; ++k) observer_destroy(this, k);
  if (xcomm) (void)ncclCommDestroy(xcomm);
  if (xstream) (void)hipStreamDestroy(xstream);
  if (rf_stream) (void)hipStreamDestroy(rf_stream);
  for (hipEvent_t e : {xev_go, xev_done, xh_ev[0], xh_ev[1], xh_ev[2], xh_ev[3], rf_done[0], rf_done[1], rf_done[2], rf_go[0], rf_go[1],
                       sreq_ev[0], sreq_ev[1], sreq_ev[2]})
    if (e) (void)hipEventDestroy(e);
  for (auto& pr : prof) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  for (void* p : {(void*)xh_host, (void*)sreq_host[0], (void*)sreq_host[1], (void*)sreq_host[2], (void*)xflag, (void*)deep_seen})
    if (p) (void)hipHostFree(p);
  if (d_pp) (void)hipFree(d_pp);
  for (void* p : allocs) (void)hipFree(p);
  for (SplitArr& A : sp) lazy_release(A.lz);
}
