// serf_sim_api.inc — part of the translation unit serf_sim.hip (included from there, in this order; not a header of its own).
// host: the C ABI of include/serf_sim.h (inside extern "C"): create / destroy, operations, the byte boundary, queries, dumps, checkpoints, profiling (stepping: serf_sim_step.inc).
#ifdef TICK_ABLATE
int sim_debug_ablate(unsigned mask) { g_ablate = mask; return SIM_OK; }
static struct AblEnv { AblEnv() { if (const char* e = getenv("SERF_ABLATE")) g_ablate = (u32)strtoul(e, nullptr, 0); } } g_abl_env;
#endif
#ifdef TICK_TIMING
int sim_debug_timing(unsigned long long* out16, int reset) {
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_tt), 32 * 8) != hipSuccess) return SIM_EDEVICE;  // (the caller's buffer holds 32 words)
  if (reset) { unsigned long long z[32] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tt), z, 32 * 8); }
  return SIM_OK;
}
#endif
uint32_t sim_abi_version(void) { return SIM_ABI_VERSION; }
const char* sim_backend_name(void) { return "hip-gfx950"; }

int sim_destroy(sim_handle* h) {
  if (!h) return SIM_EINVAL;
  delete h;  // (~sim_handle, serf_sim_host.inc)
  return SIM_OK;
}

// ---- sim_create, step by step (a step that fails returns its code: the handle's destructor gives back what the steps before it got) ----
// the Dev scalars and the handle's own parameters, from the configuration
static void create_params(sim_handle* h) {
  const sim_config* cfg = &h->cfg;
  Dev& d = h->d;
  d.N = cfg->n_nodes; d.V = cfg->vshards; d.M = d.N / d.V;
  d.sharded = cfg->shard_count > 1 || (cfg->flags & SIM_CF_FORCE_SHARDED);  // (the flag: ONE shard run as a shard — the N > 1 path with a single rank)
  d.Nl = d.sharded ? d.M : d.N;
  d.shard0 = d.sharded ? cfg->shard_rank * d.M : 0;
  d.shard_rank = cfg->shard_rank;
  h->dense = (cfg->view_slots == 0 || cfg->view_slots >= d.N);
  d.A = h->dense ? d.N : cfg->view_slots;
  d.Bev = cfg->event_ring; d.Bq = cfg->query_ring; d.f = cfg->fanout;
  d.X = cfg->ring_overflow;
  d.P = cfg->pkt_records ? cfg->pkt_records : SIM_P;
  d.PG = d.P / SIM_P;
  d.fp = d.f * d.PG;
  d.npend = d.f * d.P + SIM_S + 1u + ((cfg->flags & SIM_CF_RANDOM_FANOUT) ? SIM_RF_PEND_EXTRA : 0u);
  d.bev_mask = (d.Bev > 1 && !(d.Bev & (d.Bev - 1))) ? d.Bev - 1 : 0;
  d.bq_mask = (d.Bq > 1 && !(d.Bq & (d.Bq - 1))) ? d.Bq - 1 : 0;
  d.retransmit_mult = cfg->retransmit_mult;
  swim_params(cfg, &d.swim, &d.kconf, d.T);
  d.PI = cfg->probe_interval;
  d.ic = cfg->indirect_checks;
  d.reap_interval = cfg->reap_interval; d.reconnect_timeout = cfg->reconnect_timeout;
  d.reconnect_interval = cfg->probe_interval ? cfg->reconnect_interval : 0u;
  d.tombstone_timeout = cfg->tombstone_timeout; d.intent_timeout = cfg->intent_timeout;
  d.queue_check_interval = cfg->queue_check_interval; d.max_queue_depth = cfg->max_queue_depth;
  d.min_queue_depth = cfg->min_queue_depth;
  d.r3on = d.swim || d.reap_interval;
  d.loss_u32 = cfg->loss_u32;
  d.aw_probe = (cfg->flags & SIM_CF_AWARENESS_PROBE) ? 1u : 0u;
  d.tcp_fallback = (cfg->flags & SIM_CF_TCP_FALLBACK) ? 1u : 0u;
  d.nacks = (cfg->flags & SIM_CF_NACKS) ? 1u : 0u;
  d.gttd = cfg->gossip_to_the_dead;
  d.rfan = (cfg->flags & SIM_CF_RANDOM_FANOUT) ? 1u : 0u;
  d.prune_delay = (cfg->flags & SIM_CF_PRUNE_DELAY) ? 1u : 0u;
  h->q_timeout = 16u * h_digits10(cfg->n_nodes);  // query.rs:421-427, query_timeout_mult = 16 (options.rs:518)
  if (cfg->push_pull_interval) {  // memberlist pushPullScale: x (ceil(log2 N - 5) + 1) above 32 nodes
    u64 mult = 1;
    if (cfg->n_nodes > 32) mult = (u64)std::ceil(std::log2((double)cfg->n_nodes) - 5.0) + 1;
    u64 st = (u64)cfg->push_pull_interval * mult / PP_GROUPS;
    h->pp_step = st < 1 ? 1u : st > 0x7FFFFFFFu ? 0x7FFFFFFFu : (u32)st;
  }
  d.ev_cap = EV_CAP;
}
// the device memory that lives as long as the handle
static int create_alloc(sim_handle* h) {
  Dev& d = h->d;
  const size_t Nl = d.Nl, nup = ((size_t)d.N + 31) / 32;
  DA(d.R0, Nl) DA(d.R1, Nl) DA(d.R2, Nl) DA(d.R3, Nl) DA(d.R4, 2 * Nl) DA(d.R5, Nl)
  DA(d.qkeys, (size_t)(SIM_Q / 4u) * Nl) DA(d.qpay, (size_t)SIM_Q * Nl) DA(d.pend, (size_t)d.npend * Nl)
  DA(d.qused, Nl) DA(d.deep_list, 2 * Nl) DA(d.deep_cnt, 4)
  if (!d.sharded) {
    const size_t cu4 = d.rfan ? RF_CELL_U4 : PK_U4;  // (random fan-out: 64-byte cells, the map word inside cell 0)
    DA(d.obox[0], (size_t)d.fp * Nl * cu4) DA(d.obox[1], (size_t)d.fp * Nl * cu4)
    if (!d.rfan) { DA(d.omap[0], Nl) DA(d.omap[1], Nl) }
    DA(h->inbox_mat, (size_t)d.fp * Nl * PK_U4)
  } else if (d.rfan) {  // a shard with the random fan-out: the packets stay in their senders' cells here too (one buffer: nobody
    // reads the cells of the tick before — the receivers read the slabs the exchange delivered)
    DA(d.obox[0], (size_t)d.fp * Nl * RF_CELL_U4)
    d.obox[1] = d.obox[0];
    DA(h->inbox_mat, (size_t)d.fp * Nl * PK_U4)
  }
  // view entries and ring buckets: planes that get their memory when a slot / a Lamport time first needs them (LazyPlanes,
  // serf_sim_host.inc) where the planes are mappable units; whole otherwise
  // (the rings of a shard are whole: ev_hi / q_hi bound the cluster's clocks only when every shard hears of every record that
  // comes in over the byte boundary — slots, by contrast, are handed out by replicated bookkeeping)
  const u32 planes[SP_N] = {d.A, d.X + d.Bev, d.X + d.Bq};
  for (int i = 0; i < SP_N; ++i) {
    SplitArr& A = h->sp[i];
    A.planes = planes[i];
    A.tail = (size_t)planes[i] * Nl;
    const bool whole = i == SP_VIEW ? h->dense : d.sharded;
    if (whole || !lazy_reserve(h, A.lz, &A.base, A.planes, Nl)) DA(A.base, A.tail * 2)
  }
  // the kernels' copy
  d.view = h->sp[SP_VIEW].base; d.vtail = h->sp[SP_VIEW].tail;
  d.ering0 = h->sp[SP_EV].base; d.etail = h->sp[SP_EV].tail;
  d.qring0 = h->sp[SP_Q].base; d.qtail = h->sp[SP_Q].tail;
  d.ering = d.ering0 + (size_t)d.X * Nl; d.qring = d.qring0 + (size_t)d.X * Nl;  // bucket i = row X + i: the overflow rows come first (they are always mapped)
  DA(d.slot_of, d.N) DA(d.subject_of, d.A) DA(d.walk, d.A) DA(d.upmap, nup) DA(d.nullcell, 4) DA(d.skipmask, (d.gttd || d.rfan) ? Nl : 1) DA(h->sreq_buf[0], 1 + 2 * SIM_SUSPECT_REQ_MAX) DA(h->sreq_buf[1], 1 + 2 * SIM_SUSPECT_REQ_MAX) DA(h->sreq_buf[2], 1 + 2 * SIM_SUSPECT_REQ_MAX)
  DA(d.qtab, QTAB_U4(d.N)) DA(d.qbits, (size_t)SIM_QT * 2 * nup)
  DA(d.events, (size_t)EV_CAP) DA(d.ev_count, 1)
  DA(h->d_base, (size_t)d.N * 2)
  DA(h->d_scratch, 16)
  DA(h->d_mst, d.N)
  DA(h->d_mlt, d.N)
  DA(h->d_stats, 1)
  return SIM_OK;
}
// the state of tick 0, on the handle's stream
static int create_state(sim_handle* h) {
  const sim_config* cfg = &h->cfg;
  Dev& d = h->d;
  const size_t Nl = d.Nl, nup = ((size_t)d.N + 31) / 32;
  bool joined = cfg->flags & SIM_CF_BASELINE_JOINED;
  hipStream_t s = h->stream;
  auto zero = [&](void* p, size_t bytes) { return hipMemsetAsync(p, 0, bytes, s); };
  HCHECK(zero(d.R2, Nl * 16)); HCHECK(zero(d.R3, Nl * 16)); HCHECK(zero(d.R4, Nl * 32)); HCHECK(zero(d.R5, Nl * 16));
  HCHECK(zero(d.qpay, (size_t)SIM_Q * Nl * 16));
  HCHECK(zero(d.ev_count, 4));
  HCHECK(zero(d.nullcell, 64));
  d.sreq = h->sreq_buf[0];
  for (int i = 0; i < 3; ++i) {
    HCHECK(zero(h->sreq_buf[i], 4));
    HCHECK(hipHostMalloc((void**)&h->sreq_host[i], 2 * SREQ_HEAD * 4));
    memset(h->sreq_host[i], 0xFF, 2 * SREQ_HEAD * 4);
    HCHECK(hipEventCreateWithFlags(&h->sreq_ev[i], hipEventDisableTiming));
  }
  HCHECK(zero(d.qtab, QTAB_U4(d.N) * 16)); HCHECK(zero(d.qbits, (size_t)SIM_QT * 2 * nup * 4));
  if (!d.sharded && !d.rfan) {  // nothing has been sent yet
    HCHECK(zero(d.obox[0], (size_t)d.fp * Nl * sizeof(sim_packet))); HCHECK(zero(d.obox[1], (size_t)d.fp * Nl * sizeof(sim_packet)));
    HCHECK(hipMemsetAsync(d.omap[0], 0xFF, Nl * 4, s)); HCHECK(hipMemsetAsync(d.omap[1], 0xFF, Nl * 4, s));
  }
  if (d.rfan) {  // (all 0xFF: every map word says "nothing sent")
    HCHECK(hipMemsetAsync(d.obox[0], 0xFF, (size_t)d.fp * Nl * RF_CELL_U4 * 16, s));
    if (d.obox[1] != d.obox[0]) HCHECK(hipMemsetAsync(d.obox[1], 0xFF, (size_t)d.fp * Nl * RF_CELL_U4 * 16, s));
  }
  for (SplitArr& A : h->sp)
    if (!A.lz.va) HCHECK(zero(A.base, A.tail * 32));
  if (int rc = rings_need(h)) return rc;
  HCHECK(hipMemsetAsync(d.upmap, 0xFF, nup * 4, s));
  // base.rs:196-205: every clock starts at 1 (+ the own join at ltime 1 when pre-joined)
  fill_u4<<<grid_for(Nl), BLOCK, 0, s>>>(d.R0, Nl, make_uint4(joined ? 2 : 1, 0, 1, 0));
  fill_u4<<<grid_for(Nl), BLOCK, 0, s>>>(d.R1, Nl, make_uint4(1, 0, SIM_RF_UP | (SIM_SERF_ALIVE << 1), joined ? d.N : 1));
  fill_u4<<<grid_for((size_t)(SIM_Q / 4u) * Nl), BLOCK, 0, s>>>(d.qkeys, (size_t)(SIM_Q / 4u) * Nl, make_uint4(KEMPTY, KEMPTY, KEMPTY, KEMPTY));
  HCHECK(zero(d.deep_cnt, 16));
  HCHECK(hipHostMalloc((void**)&h->deep_seen, 4));
  *h->deep_seen = 0;
  // slot map + baseline
  h->slot_of.assign(d.N, NOSLOT);
  h->subject_of.assign(d.A, NOSLOT);
  h->alloc_tick.assign(d.A, 0);
  h->qfilt.assign((size_t)SIM_QT * SIM_QF_WORDS, 0);
  sim_view b0;
  memset(&b0, 0, sizeof b0);
  if (joined) { b0.ltime = 1; b0.bits = 1u | (SIM_STATUS_ALIVE << 1); }
  h->base.assign(d.N, b0);
  uint4 e0 = make_uint4((u32)b0.ltime, (u32)(b0.ltime >> 32), b0.inc, b0.bits), e1 = make_uint4(0, 0, 0, 0);
  fill_base<<<grid_for(d.N), BLOCK, 0, s>>>(h->d_base, d.N, e0, e1);
  if (h->dense) {
    h->n_slots = h->n_alloc = d.N;
    h->walk.resize(d.N);
    for (u32 i = 0; i < d.N; ++i) h->slot_of[i] = h->subject_of[i] = h->walk[i] = i;
    fill_iota<<<grid_for(d.N), BLOCK, 0, s>>>(d.walk, d.N);
    if (joined) {
      size_t tot = (size_t)d.A * Nl;
      fill_view_col<<<grid_for(tot), BLOCK, 0, s>>>(d.view, d.vtail, tot, 0, e0, e1);
    } else {
      init_dense_self<<<grid_for(Nl), BLOCK, 0, s>>>(d);
    }
  } else {
    h->n_slots = 0;
  }
  HCHECK(hipMemcpyAsync(d.slot_of, h->slot_of.data(), (size_t)d.N * 4, hipMemcpyHostToDevice, s));
  HCHECK(hipMemcpyAsync(d.subject_of, h->subject_of.data(), (size_t)d.A * 4, hipMemcpyHostToDevice, s));
  HCHECK(hipStreamSynchronize(s));
  HCHECK(hipGetLastError());
  return SIM_OK;
}
int sim_create(const sim_config* cfg, sim_handle** out) {
  int rc = cfg_check(cfg);
  if (rc) return rc;
  if (!out) return SIM_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
    fprintf(stderr, "serf_sim: no HIP device available (this library has no CPU fallback)\n");
    return SIM_EDEVICE;
  }
  std::unique_ptr<sim_handle> h(new sim_handle());
  h->cfg = *cfg;
  (void)hipGetDevice(&h->device);
  create_params(h.get());
  if ((rc = create_alloc(h.get())) != SIM_OK) return rc;
  if (h->d.rfan && (rc = create_rf(h.get())) != SIM_OK) return rc;
  if ((rc = create_state(h.get())) != SIM_OK) return rc;
  *out = h.release();
  return SIM_OK;
}

int sim_set_stream(sim_handle* h, void* st) {
  if (!h) return SIM_EINVAL;
  (void)hipStreamSynchronize(h->stream);
  h->stream = (hipStream_t)st;
  return SIM_OK;
}

static const uint4* cur_inbox(sim_handle* h);
static int inject_val(sim_handle* h, uint64_t tick, uint32_t op, uint32_t node, uint32_t a, uint32_t b, uint64_t val);
static void walk_upload(sim_handle* h) {  // h->walk -> d.walk (synchronous: the host vector changes again later)
  if (!h->walk.empty()) (void)hipMemcpy(h->d.walk, h->walk.data(), h->walk.size() * 4, hipMemcpyHostToDevice);
}
static int ensure_slot(sim_handle* h, u32 subject) {
  Dev& d = h->d;
  if (subject >= d.N) return SIM_EINVAL;
  if (h->slot_of[subject] != NOSLOT) return SIM_OK;
  u32 a = 0;
  while (a < d.A && h->subject_of[a] != NOSLOT) ++a;  // the lowest free slot
  if (a == d.A) return SIM_ENOSLOT;
  if (int rc = lazy_need(h, h->sp[SP_VIEW].lz, (u64)a + 1)) return rc;  // the slot's plane gets its memory now
  if (a >= h->n_slots) h->n_slots = a + 1;
  h->n_alloc++;
  h->slot_of[subject] = a;
  h->subject_of[a] = subject;
  h->alloc_tick[a] = (u32)h->tick;
  const sim_view& b = h->base[subject];
  uint4 e0 = make_uint4((u32)b.ltime, (u32)(b.ltime >> 32), b.inc, b.bits);
  uint4 e1 = make_uint4(b.conf[0], b.conf[1], b.conf[2], b.conf[3]);
  u32 pos = (u32)h->walk.size();
  while (pos > 0 && h->subject_of[h->walk[pos - 1]] > subject) --pos;
  slot_alloc_kernel<<<grid_for(d.Nl), BLOCK, 0, h->stream>>>(d.view, d.vtail, d.Nl, a, e0, e1, d.walk, (u32)h->walk.size(), pos,
                                                             d.slot_of + subject, d.subject_of + a, subject);
  h->walk.insert(h->walk.begin() + pos, a);
  return SIM_OK;
}
// the subject an operation needs a view slot for (NOSLOT: none) — SIMSPEC §2.6
static u32 op_subject(const sim_handle* h, u32 op, u32 node, u32 a, u32 b) {
  switch (op) {
    case SIM_OP_LEAVE: case SIM_OP_JOIN: case SIM_OP_LEAVE_FINISH: return node;
    case SIM_OP_FORCE_LEAVE: case SIM_OP_PRUNE: return a;
    case SIM_OP_CRASH: case SIM_OP_REVIVE: case SIM_OP_SET_TAGS: return h->d.swim ? node : NOSLOT;
    case SIM_OP_SUSPECT: return h->d.swim ? a : NOSLOT;
    case SIM_OP_DELIVER: {  // a member record from outside is about subject `a`
      u32 kind = SIM_META_KIND(b);
      if (kind == SIM_K_JOIN || kind == SIM_K_LEAVE) return a;
      return (kind >= SIM_K_ALIVE && h->d.swim) ? a : NOSLOT;
    }
    default: return NOSLOT;
  }
}

// ---- view-slot recycling (SIMSPEC §2.6; oracle recycle_*) -------------------------------------------------------------
static bool recycle_is_due(const sim_handle* h) {
  u32 R = h->cfg.recycle_interval;
  return R && !h->dense && h->tick > 0 && h->tick % R == 0 && h->recycle_at != (u32)h->tick;
}
static u32 recycle_candidates(const sim_handle* h, sim_recycle_cand* out) {
  u32 n = 0, R = h->cfg.recycle_interval, now = (u32)h->tick;
  for (u32 a = 0; a < h->n_slots; ++a) {
    if (h->subject_of[a] == NOSLOT || h->alloc_tick[a] + R > now) continue;
    u32 pos = n < SIM_RECYCLE_BATCH ? n : SIM_RECYCLE_BATCH;
    while (pos > 0 && h->alloc_tick[out[pos - 1].slot] > h->alloc_tick[a]) --pos;
    if (pos >= SIM_RECYCLE_BATCH) continue;
    u32 last = n < SIM_RECYCLE_BATCH ? n : SIM_RECYCLE_BATCH - 1;
    for (u32 i = last; i > pos; --i) out[i] = out[i - 1];
    memset(&out[pos], 0, sizeof out[pos]);
    out[pos].slot = a;
    out[pos].subject = h->subject_of[a];
    if (n < SIM_RECYCLE_BATCH) ++n;
  }
  return n;
}
static int recycle_scan(sim_handle* h, sim_recycle_cand* c, u32 n) {
  if (!n) return SIM_OK;
  Dev& d = h->d;
  hipStream_t s = h->stream;
  // (r6) the pass's device scratch is the handle's (allocated by the first pass: two hipMalloc / hipFree pairs a pass drained the device
  // each), and what comes back to the host is a word a candidate, not the N-byte table
  constexpr u32 B = SIM_RECYCLE_BATCH;
  // scr: [0] first running node | [4 .. 4 + B) slots | [4 + B ..) bad flags | [4 + 2B ..) subjects | [4 + 3B ..) "still mentioned" | the refs (16-byte aligned)
  constexpr size_t scr_words = 4 + 4 * B;
  if (!h->rc_refd) {
    if (hipMalloc((void**)&h->rc_refd, d.N) != hipSuccess) { h->rc_refd = nullptr; return SIM_ENOMEM; }
    if (hipMalloc((void**)&h->rc_scr, scr_words * 4 + B * 16) != hipSuccess) { (void)hipFree(h->rc_refd); h->rc_refd = nullptr; h->rc_scr = nullptr; return SIM_ENOMEM; }
    h->allocs.push_back(h->rc_refd);
    h->allocs.push_back(h->rc_scr);
  }
  uint8_t* refd = h->rc_refd;
  u32* scr = h->rc_scr;
  u32 hs[scr_words];
  memset(hs, 0, sizeof hs);
  hs[0] = 0xFFFFFFFFu;
  for (u32 i = 0; i < n; ++i) { hs[4 + i] = c[i].slot; hs[4 + 2 * B + i] = c[i].subject; }
  uint4* d_ref = (uint4*)(scr + scr_words);
  uint4 href[B];
  hipError_t e = hipMemsetAsync(refd, 0, d.N, s);
  if (e == hipSuccess) e = hipMemcpyAsync(scr, hs, sizeof hs, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipMemsetAsync(d_ref, 0, B * 16, s);
  if (e == hipSuccess) {
    // (random fan-out: the kernel reads the senders' cells where they lie; only a shard of the bijection has a receive buffer to look through)
    recycle_refd_kernel<<<grid_for(d.Nl), BLOCK, 0, s>>>(d, (d.sharded && !d.rfan) ? cur_inbox(h) : nullptr, (u32)(h->tick & 1), refd, scr);
    recycle_view_kernel<<<dim3((unsigned)std::min<size_t>((d.Nl + BLOCK - 1) / BLOCK, 1024), n), BLOCK, 0, s>>>(d, scr + 4, scr, d_ref, scr + 4 + B, refd, scr + 4 + 2 * B, scr + 4 + 3 * B);
    e = hipMemcpyAsync(hs, scr, sizeof hs, hipMemcpyDeviceToHost, s);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(href, d_ref, sizeof href, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  HCHECK(e);
  const u32* hbad = hs + 4 + B;
  const u32* hrefd = hs + 4 + 3 * B;
  for (u32 i = 0; i < n; ++i) {
    c[i].flags = hrefd[i] ? 1u : 0u;
    if (hs[0] == 0xFFFFFFFFu) continue;  // no running node on this shard
    memset(&c[i].ref, 0, sizeof c[i].ref);
    c[i].ref.ltime = (u64)href[i].x | ((u64)href[i].y << 32);
    c[i].ref.inc = href[i].z;
    c[i].ref.bits = href[i].w;
    c[i].flags |= 2u;
    const sim_view& r = c[i].ref;
    // settled = forgotten altogether, or known + Alive for serf and for memberlist, nothing buffered or pending
    bool settled = (r.bits == 0 && r.ltime == 0 && r.inc == 0) ||
                   ((r.bits & SIM_VB_KNOWN) && SIM_VB_STATUS(r.bits) == SIM_STATUS_ALIVE && SIM_VB_SWIM(r.bits) == SIM_SWIM_ALIVE &&
                    !SIM_VB_INTENT(r.bits) && !SIM_VB_NCONF(r.bits));
    if (!settled || hbad[i]) c[i].flags |= 1u;
  }
  return SIM_OK;
}
static int recycle_apply(sim_handle* h, const sim_recycle_cand* c, u32 n) {
  Dev& d = h->d;
  {  // a candidate that was examined and could not go goes to the back of the line (oracle recycle_apply)
    sim_recycle_cand ex[SIM_RECYCLE_BATCH];
    u32 ne = recycle_candidates(h, ex);
    for (u32 j = 0; j < ne; ++j) {
      bool agreed = false;
      for (u32 i = 0; i < n; ++i) agreed |= c[i].subject == ex[j].subject;
      if (!agreed) h->alloc_tick[ex[j].slot] = (u32)h->tick;
    }
  }
  for (u32 i = 0; i < n; ++i) {
    u32 x = c[i].subject;
    if (x >= d.N) return SIM_EINVAL;
    u32 a = h->slot_of[x];
    if (a == NOSLOT) continue;
    h->base[x] = c[i].ref;
    const sim_view& b = h->base[x];
    poke_base<<<1, 64, 0, h->stream>>>(h->d_base, x, make_uint4((u32)b.ltime, (u32)(b.ltime >> 32), b.inc, b.bits),
                                        make_uint4(b.conf[0], b.conf[1], b.conf[2], b.conf[3]));
    poke_u32<<<1, 64, 0, h->stream>>>(d.slot_of + x, NOSLOT);
    poke_u32<<<1, 64, 0, h->stream>>>(d.subject_of + a, NOSLOT);
    h->slot_of[x] = NOSLOT;
    h->subject_of[a] = NOSLOT;
    h->n_alloc--;
    h->slots_recycled++;
  }
  while (h->n_slots > 0 && h->subject_of[h->n_slots - 1] == NOSLOT) h->n_slots--;
  // the walk = the slots in use, in subject order: the freed ones drop out of it, the order stands (until r6 it was rebuilt from the
  // slot map of all N subjects — 0.3 ms of host time a pass at 1 Mi nodes, with the GPU idle behind the pass's synchronisation:
  // tools/gpu/r6_trace_pass.sh)
  h->walk.erase(std::remove_if(h->walk.begin(), h->walk.end(), [&](u32 a) { return h->subject_of[a] == NOSLOT; }), h->walk.end());
  HCHECK(hipStreamSynchronize(h->stream));
  walk_upload(h);
  return SIM_OK;
}
static int recycle_local(sim_handle* h) {  // every shard is in this process: decide here
  sim_recycle_cand c[SIM_RECYCLE_BATCH];
  u32 n = recycle_candidates(h, c), m = 0;
  int rc = recycle_scan(h, c, n);
  if (rc) return rc;
  for (u32 i = 0; i < n; ++i)
    if ((c[i].flags & 3u) == 2u) c[m++] = c[i];
  rc = recycle_apply(h, c, m);
  h->recycle_at = (u32)h->tick;
  return rc;
}
// what an operation's arguments have to satisfy before it may reach ops_kernel (sim_inject, and every pending operation
// of an image being restored)
static int op_validate(u32 N, u32 op, u32 node, u32 a, u32 b) {
  if (node >= N) return SIM_EINVAL;
  switch (op) {
    case SIM_OP_USER_EVENT: if (!a) return SIM_EINVAL; if ((b & 0x7FFFFFFFu) > 9 * 1024) return SIM_ETOOBIG; break;  // bit 31: cc
    case SIM_OP_QUERY: if (!a) return SIM_EINVAL; break;
    case SIM_OP_LEAVE: case SIM_OP_JOIN: case SIM_OP_LEAVE_FINISH: case SIM_OP_CRASH: case SIM_OP_REVIVE: break;
    case SIM_OP_FORCE_LEAVE: if (a >= N) return SIM_EINVAL; break;
    case SIM_OP_SET_TAGS: if (a >= SIM_TAG_CLASSES) return SIM_EINVAL; break;
    case SIM_OP_QUERY_FILTER_ID: if (!a || b >= N) return SIM_EINVAL; break;
    case SIM_OP_QUERY_FILTER_TAGS: if (!a) return SIM_EINVAL; break;
    case SIM_OP_SUSPECT: case SIM_OP_RECONNECT: case SIM_OP_PRUNE: if (a >= N) return SIM_EINVAL; break;
    case SIM_OP_DELIVER: {
      u32 kind = SIM_META_KIND(b);
      if (kind < SIM_K_JOIN || kind > SIM_K_DEAD || (b & ~(SIM_META_WIRE_MASK | SIM_DELIVER_MUTE))) return SIM_EINVAL;
      if ((b & SIM_DELIVER_MUTE) && kind != SIM_K_JOIN && kind != SIM_K_LEAVE && kind != SIM_K_EVENT) return SIM_EINVAL;
      if (kind == SIM_K_EVENT || kind == SIM_K_QUERY) { if (!a) return SIM_EINVAL; }
      else if (a >= N) return SIM_EINVAL;
      break;
    }
    case SIM_OP_QRESP: if (!a || (b & 0xFFFFFFu) >= N || (b & 0x7F000000u)) return SIM_EINVAL; break;
    case SIM_OP_WITNESS: if (a > 2u) return SIM_EINVAL; break;
    default: return SIM_EINVAL;
  }
  return SIM_OK;
}
static int inject_val(sim_handle* h, uint64_t tick, uint32_t op, uint32_t node, uint32_t a, uint32_t b, uint64_t val) {
  if (!h) return SIM_EINVAL;
  if (tick < h->tick) tick = h->tick;
  if (op == SIM_OP_SUSPECT && (a & SREQ_RECONNECT)) { op = SIM_OP_RECONNECT; a &= ~SREQ_RECONNECT; }  // an entry of the request list, as it stands there
  else if (op == SIM_OP_SUSPECT && (a & SREQ_PRUNE)) {  // ... of a pruning leave intent: due leave_delay ticks after the tick it was noted in — the list is read two ticks after
    op = SIM_OP_PRUNE; a &= ~SREQ_PRUNE;
    if (h->cfg.leave_delay > 2) tick += h->cfg.leave_delay - 2;
  }
  int rc = op_validate(h->d.N, op, node, a, b);
  if (rc) return rc;
  // an operation that executes now gets its view slot now (and SIM_ENOSLOT if there is none); one scheduled for a
  // later tick gets it when it executes — and is dropped and counted if none is free then (SIMSPEC §2.6)
  // (a SIM_OP_SUSPECT always takes its slot when it executes: it is scheduled by the library / the sharded host, and a
  // full view must count it as dropped the same way in both)
  if (op != SIM_OP_SUSPECT && tick <= h->tick && op_subject(h, op, node, a, b) != NOSLOT) rc = ensure_slot(h, op_subject(h, op, node, a, b));
  if (rc) return rc;
  // the ring planes this operation can make a record reach (LazyPlanes: ev_hi / q_hi bound every clock)
  if (op == SIM_OP_USER_EVENT) h->ev_hi++;
  else if (op == SIM_OP_QUERY) h->q_hi++;
  else if (op == SIM_OP_DELIVER && SIM_META_KIND(b) == SIM_K_EVENT) h->ev_hi = std::max<u64>(h->ev_hi, std::min<u64>(val, ~0ull - 4) + 1);
  else if (op == SIM_OP_DELIVER && SIM_META_KIND(b) == SIM_K_QUERY) h->q_hi = std::max<u64>(h->q_hi, std::min<u64>(val, ~0ull - 4) + 1);
  else if (op == SIM_OP_WITNESS && a == 1u) h->ev_hi = std::max<u64>(h->ev_hi, std::min<u64>(val, ~0ull - 4) + 1);
  else if (op == SIM_OP_WITNESS && a == 2u) h->q_hi = std::max<u64>(h->q_hi, std::min<u64>(val, ~0ull - 4) + 1);
  if ((rc = rings_need(h)) != SIM_OK) return rc;
  size_t pos = h->ops.size();
  h->ops.push_back(OpEnt{tick, op, node, a, b, val});
  // order within a tick: the operations in the order they were scheduled, then the suspicions / reconnect attempts the
  // library replays from the request lists (SIM_OP_SUSPECT / SIM_OP_RECONNECT) in theirs.  The replay happens at sim_step_begin,
  // behind everything the caller has scheduled for the tick — unless a checkpoint (sim_snapshot) or the sharded host's hand-over
  // put the lists into the schedule earlier: what the caller schedules for the same tick afterwards still goes first
  // (ADVICE r4: taking a checkpoint changed the order of a tick's operations).
  auto late = [](u32 o) { return o == SIM_OP_SUSPECT || o == SIM_OP_RECONNECT || o == SIM_OP_PRUNE; };
  while (pos > h->op_cursor && (h->ops[pos - 1].tick > tick || (h->ops[pos - 1].tick == tick && late(h->ops[pos - 1].op) && !late(op)))) {
    std::swap(h->ops[pos], h->ops[pos - 1]);
    --pos;
  }
  return SIM_OK;
}
int sim_inject(sim_handle* h, uint64_t tick, uint32_t op, uint32_t node, uint32_t a, uint32_t b) {
  if (op == SIM_OP_DELIVER || op == SIM_OP_QRESP || op == SIM_OP_WITNESS) return SIM_EINVAL;  // internal, with a value: sim_inject_record / sim_deliver_message
  return inject_val(h, tick, op, node, a, b, 0);
}
// ---- the byte boundary of the delegate (include/serf_sim.h; oracle: the same entry points with its own C codec) ----
int sim_inject_record(sim_handle* h, uint64_t tick, uint32_t node, const sim_record* rec) {
  if (!h || !rec) return SIM_EINVAL;
  return inject_val(h, tick, SIM_OP_DELIVER, node, rec->key, rec->meta & SIM_META_WIRE_MASK, rec->val);
}
int sim_user_event_bytes(sim_handle* h, uint32_t node, const uint8_t* name, size_t nlen, const uint8_t* payload, size_t plen, int cc) {
  if (!h || (nlen && !name) || (plen && !payload)) return SIM_EINVAL;
  if (nlen + plen > 512) return SIM_ETOOBIG;  // api.rs:246-262 user_event_size_limit
  namespace w = serf::wire;
  w::Bytes nm(name, name + nlen), pl(payload, payload + plen);
  u32 key = w::event_key(nm, pl);
  h->evreg.emplace(key, std::make_pair(nm, pl));  // the first content under a key stays
  return sim_user_event(h, node, key, (uint32_t)w::user_event_len(1, nm, pl, cc != 0), cc);
}
// `relayed`: the message is the inside of a Relay
static int deliver_one(sim_handle* h, uint32_t node, const uint8_t* buf, size_t len, size_t* consumed, bool relayed) {
  if (!h || !buf || !len || node >= h->d.N) return SIM_EINVAL;
  namespace w = serf::wire;
  try {
    w::Bytes in(buf, buf + len);
    if (in[0] == w::merge(w::WIRE_LEN, w::RELAY)) {
      // Relay (types/message.rs:431-470): `node` forwards the wrapped message to the node it names as it is (delegate.rs:262-313:
      // memberlist.send) — if it is running; a process that is down forwards nothing
      if (relayed) return SIM_EINVAL;
      auto [dest, off] = w::unwrap_relay(in);
      if (dest >= h->d.N || off >= len) return SIM_EINVAL;
      const u32 in_tag = buf[off] >> 3;
      if (in_tag == w::PUSH_PULL || in_tag == w::RELAY) return SIM_EINVAL;  // a push-pull does not travel as a user message; no nesting
      u32 word = 0;  // ground-truth liveness as of the end of the last tick (rare call: one word, one wait)
      HCHECK(hipMemcpyAsync(&word, h->d.upmap + (node >> 5), 4, hipMemcpyDeviceToHost, h->stream));
      HCHECK(hipStreamSynchronize(h->stream));
      size_t in_used = 0;
      int rc = SIM_OK;
      if ((word >> (node & 31)) & 1u) rc = deliver_one(h, dest, buf + off, len - off, &in_used, true);
      else {  // dropped with its relay: the inner frame is still walked so that the caller learns its length
        w::Bytes inner(buf + off, buf + len);
        (void)w::unframe(inner, in_used);
      }
      if (rc == SIM_OK && consumed) *consumed = off + in_used;
      return rc;
    }
    size_t used = 0;
    auto [tag, body] = w::unframe(in, used);
    sim_record rec;
    memset(&rec, 0, sizeof rec);
    int rc = SIM_OK;
    if (tag == w::QUERY_RESPONSE) {  // -> SIM_OP_QRESP at the origin
      w::QueryResponse m = w::decode_query_response(body);
      if (m.from_node >= h->d.N || !m.id) return SIM_EINVAL;
      rc = inject_val(h, h->tick, SIM_OP_QRESP, node, m.id, m.from_node | ((m.flags & 1u) ? 0x80000000u : 0u), 0);
      if (rc == SIM_OK && consumed) *consumed = used;
      return rc;
    }
    if (tag == w::CONFLICT_RESPONSE) {  // notify_message has no arm for it ("receive unexpected message type", delegate.rs:286-288)
      if (consumed) *consumed = used;
      return SIM_OK;
    }
    if (tag == w::PUSH_PULL) {  // what merge_remote_state (delegate.rs:427-554) does with it
      w::PushPull m = w::decode_push_pull(body);
      for (auto& st : m.status_ltimes)
        if (st.first >= h->d.N) return SIM_EINVAL;
      for (u32 id : m.left_members)
        if (id >= h->d.N) return SIM_EINVAL;
      {  // a frame that is refused leaves NOTHING behind: the view slots its members need (they execute in this tick) are counted first
        std::vector<u32> need;
        for (auto& st : m.status_ltimes)
          if (h->slot_of[st.first] == NOSLOT && std::find(need.begin(), need.end(), st.first) == need.end()) need.push_back(st.first);
        if (need.size() > (size_t)(h->d.A - h->n_alloc)) return SIM_ENOSLOT;
      }
      const u64 clk[3] = {m.ltime, m.event_ltime, m.query_ltime};
      for (u32 i = 0; i < 3 && rc == SIM_OK; ++i)  // "we subtract 1 since no message with that clock has been sent yet"
        if (clk[i] > 0) rc = inject_val(h, h->tick, SIM_OP_WITNESS, node, i, 0, clk[i] - 1);
      auto is_left = [&](u32 id) { return std::find(m.left_members.begin(), m.left_members.end(), id) != m.left_members.end(); };
      for (size_t i = 0; i < m.left_members.size() && rc == SIM_OK; ++i) {  // the left members first, one past their status time
        size_t j = 0;
        while (j < m.status_ltimes.size() && m.status_ltimes[j].first != m.left_members[i]) ++j;
        if (j < m.status_ltimes.size())
          rc = inject_val(h, h->tick, SIM_OP_DELIVER, node, m.left_members[i], wire_meta(SIM_K_LEAVE, 0, 16) | SIM_DELIVER_MUTE, m.status_ltimes[j].second + 1);
      }
      for (size_t j = 0; j < m.status_ltimes.size() && rc == SIM_OK; ++j)  // every other member: an artificial join message at its status time
        if (!is_left(m.status_ltimes[j].first))
          rc = inject_val(h, h->tick, SIM_OP_DELIVER, node, m.status_ltimes[j].first, wire_meta(SIM_K_JOIN, 0, 16) | SIM_DELIVER_MUTE, m.status_ltimes[j].second);
      for (auto& bucket : m.events)  // the event buffer, replayed in order
        for (auto& ev : bucket.second) {
          if (rc != SIM_OK) break;
          u32 key = w::event_key(ev.first, ev.second);
          h->evreg.emplace(key, std::make_pair(ev.first, ev.second));
          rc = inject_val(h, h->tick, SIM_OP_DELIVER, node, key, wire_meta(SIM_K_EVENT, 0, 32) | SIM_DELIVER_MUTE, bucket.first);
        }
      if (rc == SIM_OK && consumed) *consumed = used;
      return rc;
    }
    if (tag == w::JOIN) {
      w::Join m = w::decode_join(body);
      if (m.id >= h->d.N) return SIM_EINVAL;
      rec.key = m.id; rec.val = m.ltime; rec.meta = wire_meta(SIM_K_JOIN, 0, (u32)used);
    } else if (tag == w::LEAVE) {
      w::Leave m = w::decode_leave(body);
      if (m.id >= h->d.N) return SIM_EINVAL;
      rec.key = m.id; rec.val = m.ltime; rec.meta = wire_meta(SIM_K_LEAVE, m.prune ? SIM_F_PRUNE : 0, (u32)used);
    } else if (tag == w::USER_EVENT) {
      w::UserEvent m = w::decode_user_event(body);
      rec.key = w::event_key(m.name, m.payload); rec.val = m.ltime;
      rec.meta = wire_meta(SIM_K_EVENT, m.cc ? SIM_F_CC : 0, (u32)used);
      h->evreg.emplace(rec.key, std::make_pair(m.name, m.payload));
    } else if (tag == w::QUERY) {
      w::Query m = w::decode_query(body);
      if (!m.id) return SIM_EINVAL;
      rec.key = m.id; rec.val = m.ltime;
      rec.meta = wire_meta(SIM_K_QUERY, ((m.flags & 1u) ? SIM_F_ACK : 0u) | ((m.flags & 2u) ? SIM_F_NO_BROADCAST : 0u), 48);  // every query is priced at 48 B
      std::vector<u32> ids;
      for (const w::Bytes& f : m.filters) {  // types/filter.rs:176-262: Id = (id_byte <id>)*, Tag = tag_byte <TagFilter>
        size_t off = 0;
        while (off < f.size()) {
          if ((f[off++] >> 3) != 1) return SIM_EINVAL;  // a tag expression: evaluated by the host (sim_query_filtered)
          u32 g = w::parse_node_id(w::read_ld(f, off));
          if (g >= h->d.N || ids.size() == SIM_QF_IDS) return SIM_EINVAL;
          ids.push_back(g);
        }
      }
      for (u32 g : ids)
        if ((rc = inject_val(h, h->tick, SIM_OP_QUERY_FILTER_ID, node, rec.key, g, 0)) != SIM_OK) return rc;
    } else {
      return SIM_EINVAL;  // not a message of the simulated path
    }
    rc = sim_inject_record(h, h->tick, node, &rec);
    if (rc == SIM_OK && consumed) *consumed = used;
    return rc;
  } catch (const std::exception&) {
    return SIM_EINVAL;
  }
}
int sim_deliver_message(sim_handle* h, uint32_t node, const uint8_t* buf, size_t len, size_t* consumed) {
  return deliver_one(h, node, buf, len, consumed, false);
}
int sim_join(sim_handle* h, uint32_t node, uint32_t peer) { return sim_inject(h, h ? h->tick : 0, SIM_OP_JOIN, node, peer, 0); }
int sim_leave(sim_handle* h, uint32_t node) {
  if (!h) return SIM_EINVAL;
  // api.rs:422-499: leave intent now; memberlist.leave after broadcast_timeout; the caller's
  // shutdown() (api.rs:525) after leave_propagate_delay — both modelled as leave_delay ticks
  int rc = sim_inject(h, h->tick, SIM_OP_LEAVE, node, 0, 0);
  if (rc) return rc;
  rc = sim_inject(h, h->tick + h->cfg.leave_delay + 1, SIM_OP_LEAVE_FINISH, node, 0, 0);
  if (rc) return rc;
  return sim_inject(h, h->tick + 2 * h->cfg.leave_delay + 2, SIM_OP_CRASH, node, 0, 0);
}
int sim_force_leave(sim_handle* h, uint32_t node, uint32_t subject, int prune) {
  return sim_inject(h, h ? h->tick : 0, SIM_OP_FORCE_LEAVE, node, subject, prune ? 1u : 0u);
}
int sim_user_event(sim_handle* h, uint32_t node, uint32_t key, uint32_t len, int cc) {
  // UserEventMessage.cc (types/user_event/message.rs) travels in the record's flag bits
  return sim_inject(h, h ? h->tick : 0, SIM_OP_USER_EVENT, node, key, (len & 0x7FFFFFFFu) | (cc ? 0x80000000u : 0u));
}
int sim_query(sim_handle* h, uint32_t node, uint32_t id, uint32_t flags) {
  return sim_inject(h, h ? h->tick : 0, SIM_OP_QUERY, node, id, flags);
}
int sim_query_filtered(sim_handle* h, uint32_t node, uint32_t id, uint32_t flags, const uint32_t* ids, uint32_t n_ids, uint32_t tag_mask) {
  if (!h || !id || node >= h->d.N || (n_ids && !ids)) return SIM_EINVAL;
  if (n_ids > SIM_QF_IDS) return SIM_ETOOBIG;
  for (u32 i = 0; i < n_ids; ++i)
    if (ids[i] >= h->d.N) return SIM_EINVAL;
  int rc = SIM_OK;
  for (u32 i = 0; i < n_ids && rc == SIM_OK; ++i) rc = sim_inject(h, h->tick, SIM_OP_QUERY_FILTER_ID, node, id, ids[i]);
  if (rc == SIM_OK && tag_mask != 0xFFFFFFFFu) rc = sim_inject(h, h->tick, SIM_OP_QUERY_FILTER_TAGS, node, id, tag_mask);
  return rc ? rc : sim_inject(h, h->tick, SIM_OP_QUERY, node, id, flags);
}
int sim_init_tags(sim_handle* h, uint32_t first, uint32_t count, const uint8_t* classes) {
  if (!h || !classes || first > h->d.N || count > h->d.N - first) return SIM_EINVAL;
  for (u32 i = 0; i < count; ++i)
    if (classes[i] >= SIM_TAG_CLASSES) return SIM_EINVAL;
  if (!count) return SIM_OK;
  HCHECK(hipMemcpyAsync(TAGCLASS(h->d) + first, classes, count, hipMemcpyHostToDevice, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));  // the caller's buffer is free again when this returns
  return SIM_OK;
}
int sim_set_tags(sim_handle* h, uint32_t node, uint32_t tag_class) {
  return sim_inject(h, h ? h->tick : 0, SIM_OP_SET_TAGS, node, tag_class, 0);
}

// ---- cross-shard push-pull, driven by the sharded host (include/serf_sim.h; oracle pp_plan / pp_export / pp_merge) ----
static bool pp_batch_class(const sim_handle* h, u32* cls) {
  if (!h->pp_step || h->tick == 0 || h->tick % h->pp_step) return false;
  *cls = (u32)((h->tick / h->pp_step) % PP_GROUPS);
  return true;
}
int sim_pp_due(const sim_handle* h) {
  u32 cls;
  if (!h) return SIM_EINVAL;
  // (a reconnect attempt is a push-pull pair as well: known once sim_step_begin has resolved the tick's operations)
  return (h->d.sharded && (pp_batch_class(h, &cls) || (h->in_tick && !h->rc_a.empty())) && h->pp_done_at != (u32)h->tick) ? 1 : 0;
}
int sim_pp_plan(sim_handle* h, uint32_t* send1, uint32_t* recv1, size_t* record_bytes) {
  u32 cls = 0;
  if (!h || !send1 || !recv1 || !record_bytes) return SIM_EINVAL;
  const bool batch = h->in_tick && pp_batch_class(h, &cls);
  if (!h->in_tick || !h->d.sharded || (!batch && h->rc_a.empty())) return SIM_ESTATE;  // after sim_step_begin: the tick's operations come first
  Dev& d = h->d;
  const TickP& tp = h->cur_tp;
  const u32 V = d.V, me = d.shard_rank, M = d.M;
  std::vector<u32> up(((size_t)d.N + 31) / 32);  // ground-truth liveness after this tick's operations
  HCHECK(hipMemcpyAsync(up.data(), d.upmap, up.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  auto is_up = [&](u32 g) { return (up[g >> 5] >> (g & 31)) & 1u; };
  for (u32 v = 0; v < V; ++v) send1[v] = recv1[v] = 0;
  h->pp_local_a.clear(); h->pp_local_b.clear();
  std::vector<std::vector<u32>> r1(V), s1(V);
  auto place = [&](u32 ga, u32 gb) {
    if (!is_up(ga) || !is_up(gb)) return;
    u32 oa = ga / M, ob = gb / M;
    if (oa == me && ob == me) { h->pp_local_a.push_back(ga - d.shard0); h->pp_local_b.push_back(gb - d.shard0); }
    else if (oa == me) r1[ob].push_back(ga - d.shard0);
    else if (ob == me) s1[oa].push_back(gb - d.shard0);
  };
  if (batch)
    for (u32 pi = cls; 2 * (u64)pi + 1 < tp.N; pi += PP_GROUPS) place(sigma_g_inv(tp, 2 * pi), sigma_g_inv(tp, 2 * pi + 1));
  else  // the tick's reconnect attempts (sim_step_begin): the initiator is `a`, it merges first
    for (size_t i = 0; i < h->rc_a.size(); ++i) place(h->rc_a[i], h->rc_b[i]);
  h->pp_r1.clear(); h->pp_s1.clear();
  for (u32 v = 0; v < V; ++v) {
    recv1[v] = (u32)r1[v].size(); send1[v] = (u32)s1[v].size();
    h->pp_r1.insert(h->pp_r1.end(), r1[v].begin(), r1[v].end());
    h->pp_s1.insert(h->pp_s1.end(), s1[v].begin(), s1[v].end());
  }
  // the four lists on the device: local a | local b | r1 | s1
  size_t tot = h->pp_local_a.size() * 2 + h->pp_r1.size() + h->pp_s1.size();
  if (h->d_pp) { (void)hipFree(h->d_pp); h->d_pp = nullptr; }
  if (tot) {
    if (hipMalloc((void**)&h->d_pp, tot * 4) != hipSuccess) return SIM_ENOMEM;
    std::vector<u32> all;
    all.reserve(tot);
    all.insert(all.end(), h->pp_local_a.begin(), h->pp_local_a.end());
    all.insert(all.end(), h->pp_local_b.begin(), h->pp_local_b.end());
    all.insert(all.end(), h->pp_r1.begin(), h->pp_r1.end());
    all.insert(all.end(), h->pp_s1.begin(), h->pp_s1.end());
    HCHECK(hipMemcpy(h->d_pp, all.data(), tot * 4, hipMemcpyHostToDevice));
  }
  *record_bytes = (2 + (size_t)tp.n_slots + 2 * (size_t)h->sp[SP_EV].planes) * 16;
  return SIM_OK;
}
int sim_pp_export(sim_handle* h, int round, void* send) {
  if (!h || (round != 1 && round != 2)) return SIM_EINVAL;
  if (!h->in_tick || !h->d.sharded) return SIM_ESTATE;
  Dev& d = h->d;
  const TickP& tp = h->cur_tp;
  size_t nl = h->pp_local_a.size();
  const u32* list = h->d_pp + 2 * nl + (round == 1 ? h->pp_r1.size() : 0);
  u32 n = (u32)(round == 1 ? h->pp_s1.size() : h->pp_r1.size());
  if (!n) return SIM_OK;
  if (!send) return SIM_EINVAL;
  size_t rec_u4 = 2 + (size_t)tp.n_slots + 2 * (size_t)h->sp[SP_EV].planes;
  pp_export_kernel<<<n, 256, 0, h->stream>>>(d, list, tp.n_slots, (uint4*)send, rec_u4);
  HCHECK(hipGetLastError());
  return SIM_OK;
}
int sim_pp_merge(sim_handle* h, int round, const void* recv) {
  if (!h || (round != 1 && round != 2)) return SIM_EINVAL;
  if (!h->in_tick || !h->d.sharded) return SIM_ESTATE;
  Dev& d = h->d;
  const TickP& tp = h->cur_tp;
  size_t nl = h->pp_local_a.size();
  size_t rec_u4 = 2 + (size_t)tp.n_slots + 2 * (size_t)h->sp[SP_EV].planes;
  if (round == 1) {
    if (nl) pp_local_kernel<<<(unsigned)((nl + 63) / 64), 64, 0, h->stream>>>(d, tp, h->d_pp, h->d_pp + nl, (u32)nl);
    u32 n = (u32)h->pp_r1.size();
    if (n && !recv) return SIM_EINVAL;
    if (n) pp_cross_kernel<<<(n + 63) / 64, 64, 0, h->stream>>>(d, tp, h->d_pp + 2 * nl, n, (const uint4*)recv, rec_u4);
  } else {
    u32 n = (u32)h->pp_s1.size();
    if (n && !recv) return SIM_EINVAL;
    if (n) pp_cross_kernel<<<(n + 63) / 64, 64, 0, h->stream>>>(d, tp, h->d_pp + 2 * nl + h->pp_r1.size(), n, (const uint4*)recv, rec_u4);
    h->pp_done_at = (u32)h->tick;
  }
  HCHECK(hipGetLastError());
  return SIM_OK;
}
int sim_recycle_due(const sim_handle* h) { return h ? (recycle_is_due(h) ? 1 : 0) : SIM_EINVAL; }
int sim_recycle_scan(sim_handle* h, sim_recycle_cand* out, uint32_t cap, uint32_t* n) {
  if (!h || !out || !n || cap < SIM_RECYCLE_BATCH) return SIM_EINVAL;
  if (h->in_tick) return SIM_ESTATE;
  *n = recycle_candidates(h, out);
  return recycle_scan(h, out, *n);
}
int sim_recycle_apply(sim_handle* h, const sim_recycle_cand* agreed, uint32_t n) {
  if (!h || (n && !agreed)) return SIM_EINVAL;
  if (h->in_tick) return SIM_ESTATE;
  int rc = recycle_apply(h, agreed, n);
  h->recycle_at = (u32)h->tick;
  return rc;
}
int sim_tick(const sim_handle* h, uint64_t* t) {
  if (!h || !t) return SIM_EINVAL;
  *t = h->tick;
  return SIM_OK;
}

int sim_members(sim_handle* h, uint32_t obs, uint8_t* st, uint64_t* lt, uint32_t cap) {
  if (!h) return SIM_EINVAL;
  Dev& d = h->d;
  if (obs < d.shard0 || obs >= d.shard0 + d.Nl) return SIM_EINVAL;
  if (cap < d.N) return SIM_ERANGE;
  members_kernel<<<grid_for(d.N), BLOCK, 0, h->stream>>>(d, h->d_base, obs - d.shard0, h->d_mst, h->d_mlt);
  if (st) HCHECK(hipMemcpyAsync(st, h->d_mst, d.N, hipMemcpyDeviceToHost, h->stream));
  if (lt) HCHECK(hipMemcpyAsync(lt, h->d_mlt, (size_t)d.N * 8, hipMemcpyDeviceToHost, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return SIM_OK;
}
int sim_stats_get(sim_handle* h, uint32_t node, sim_stats* o) {
  if (!h || !o) return SIM_EINVAL;
  Dev& d = h->d;
  if (node < d.shard0 || node >= d.shard0 + d.Nl) return SIM_EINVAL;
  stats_kernel<<<1, 64, 0, h->stream>>>(d, node - d.shard0, h->d_stats);
  HCHECK(hipMemcpyAsync(o, h->d_stats, sizeof(sim_stats), hipMemcpyDeviceToHost, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return SIM_OK;
}
int sim_watch(sim_handle* h, uint32_t obs) {
  if (!h) return SIM_EINVAL;
  Dev& d = h->d;
  if (obs < d.shard0 || obs >= d.shard0 + d.Nl) return SIM_EINVAL;
  set_flag_bits<<<1, 64, 0, h->stream>>>(d.R1, obs - d.shard0, SIM_RF_WATCHED);
  return SIM_OK;
}
int sim_drain_events(sim_handle* h, sim_event* out, uint32_t cap, uint32_t* n) {
  if (!h || !n) return SIM_EINVAL;
  Dev& d = h->d;
  HCHECK(hipStreamSynchronize(h->stream));
  u32 cnt = 0;
  HCHECK(hipMemcpy(&cnt, d.ev_count, 4, hipMemcpyDeviceToHost));
  if (cnt > d.ev_cap) { h->events_lost += cnt - d.ev_cap; cnt = d.ev_cap; }
  std::vector<sim_event> ev(cnt);
  if (cnt) HCHECK(hipMemcpy(ev.data(), d.events, (size_t)cnt * sizeof(sim_event), hipMemcpyDeviceToHost));
  // per node the log is in program order; across nodes the oracle's order is (tick, observer)
  std::stable_sort(ev.begin(), ev.end(), [](const sim_event& a, const sim_event& b) {
    return a.tick != b.tick ? a.tick < b.tick : a.observer < b.observer;
  });
  u32 m = std::min(cnt, cap);
  if (out && m) memcpy(out, ev.data(), (size_t)m * sizeof(sim_event));
  // keep what did not fit
  u32 rest = cnt - m;
  if (rest) HCHECK(hipMemcpy(d.events, ev.data() + m, (size_t)rest * sizeof(sim_event), hipMemcpyHostToDevice));
  HCHECK(hipMemcpy(d.ev_count, &rest, 4, hipMemcpyHostToDevice));
  *n = m;
  return SIM_OK;
}

// The packets in flight, receiver-indexed ([f][Nl] cells).  Sharded: the receive buffer.  Local mode: Dev::obox turned
// inside out on h->stream (every user launches on that stream afterwards); the map is the one of the tick they were sent in.
static const uint4* cur_inbox(sim_handle* h) {
  if (h->xcomm && h->xpending) (void)sim_exchange_wait(h);  // (what the exchange stream still holds — the round's packets, the pack of this shard's own slab — comes first)
  if (h->d.sharded && !h->d.rfan) return h->rbuf[(h->tick + 1) & 1];
  if (h->mat_tick != h->tick) {
    const Dev& d = h->d;
    TickP p;
    tickp_make(&p, &h->cfg, h->tick ? h->tick - 1 : 0);
    materialize_kernel<<<grid_for((size_t)d.fp * d.Nl), BLOCK, 0, h->stream>>>(d, p, (u32)(h->tick & 1), h->tick ? 1u : 0u, h->inbox_mat);
    h->mat_tick = h->tick;
  }
  return h->inbox_mat;
}
int sim_state_digest(sim_handle* h, uint64_t out[8]) {
  if (!h || !out) return SIM_EINVAL;
  Dev& d = h->d;
  hipStream_t s = h->stream;
  HCHECK(hipMemsetAsync(h->d_scratch, 0, 16 * 8, s));
  digest_rows_queue<<<grid_for(d.Nl), BLOCK, 0, s>>>(d, h->d_scratch + 0, h->d_scratch + 1);
  size_t nw;
  if (cur_inbox(h)) { nw = (size_t)d.fp * d.Nl * (sizeof(sim_packet) / 8); digest_flat<<<grid_for(nw), BLOCK, 0, s>>>((const u64*)cur_inbox(h), nw, h->d_scratch + 2); }
  // (planes without memory are the zeros they stand for: their share of the sum is a function of the word indices alone)
  for (int i = 0; i < SP_N; ++i) {  // words 3, 4, 5: view, event ring, query ring
    const SplitArr& A = h->sp[i];
    const size_t have = (size_t)split_mapped(A) * d.Nl;
    if (have) digest_split<<<grid_for(have), BLOCK, 0, s>>>(A.base, A.tail, have, h->d_scratch + 3 + i);
    if (have < A.tail) digest_split_zero<<<grid_for(A.tail - have), BLOCK, 0, s>>>(have, A.tail, h->d_scratch + 3 + i);
  }
  digest_aux<<<grid_for((size_t)d.N + d.N / 32 + 1), BLOCK, 0, s>>>(d.slot_of, d.upmap, d.N, h->d_scratch + 6);
  nw = (size_t)SIM_QT * 2 * (((size_t)d.N + 31) / 32);
  digest_queries<<<grid_for(nw + 2 * SIM_QT + SIM_QT * SIM_QF_WORDS + d.N), BLOCK, 0, s>>>(d.qtab, d.qbits, nw, d.N, h->d_scratch + 7);
  HCHECK(hipMemcpyAsync(out, h->d_scratch, 8 * 8, hipMemcpyDeviceToHost, s));
  HCHECK(hipStreamSynchronize(s));
  if (h->xflag && *h->xflag) return SIM_ERANGE;  // (the state digested is that of a run whose exchange lost packets: say so)
  return SIM_OK;
}

// Split arrays (view, rings) <-> their canonical interleaved form, in chunks of at most 64 MiB of device scratch
// (only the planes that have memory — LazyPlanes — are copied; the rest of a download is zeros, the rest of an upload is not sent:
// the caller has seen to it that it is zeros)
static_assert(sizeof(sim_view) == 32 && sizeof(sim_bucket) == 32, "an entry of a split array: two 16-byte halves");
static int split_copy(sim_handle* h, const SplitArr& A, void* host, bool download) {
  const size_t CH = (size_t)1 << 21;  // entries per chunk
  const size_t n_entries = (size_t)split_mapped(A) * h->d.Nl;
  if (download && n_entries < A.tail) memset((uint8_t*)host + n_entries * 32, 0, (A.tail - n_entries) * 32);
  if (!n_entries) return SIM_OK;
  DevScratch<uint4> tmp;  // 2 x 16 bytes an entry
  if (int rc = tmp.alloc(std::min(n_entries, CH) * 2)) return rc;
  for (size_t first = 0; first < n_entries; first += CH) {
    size_t cnt = std::min(CH, n_entries - first);
    uint8_t* hp = (uint8_t*)host + first * 32;
    if (download) {
      canon_entries_kernel<<<grid_for(cnt), BLOCK, 0, h->stream>>>(A.base, A.tail, first, cnt, tmp.get());
      HCHECK(hipMemcpyAsync(hp, tmp.get(), cnt * 32, hipMemcpyDeviceToHost, h->stream));
    } else {
      HCHECK(hipMemcpyAsync(tmp.get(), hp, cnt * 32, hipMemcpyHostToDevice, h->stream));
      uncanon_entries_kernel<<<grid_for(cnt), BLOCK, 0, h->stream>>>(A.base, A.tail, first, cnt, tmp.get());
    }
    HCHECK(hipStreamSynchronize(h->stream));  // tmp is reused by the next chunk (and freed behind the last)
  }
  return SIM_OK;
}
int sim_dump_state(sim_handle* h, uint32_t which, void* buf, size_t cap, size_t* bytes) {
  if (!h || !bytes) return SIM_EINVAL;
  Dev& d = h->d;
  size_t Nl = d.Nl, n;
  const void* src = nullptr;
  switch (which) {
    case SIM_ARR_ROWS: n = Nl * sizeof(sim_row); break;
    case SIM_ARR_QUEUE: n = Nl * SIM_Q * sizeof(sim_record); break;
    case SIM_ARR_INBOX: src = cur_inbox(h); n = (size_t)d.fp * Nl * sizeof(sim_packet); break;
    case SIM_ARR_VIEW: case SIM_ARR_ERING: case SIM_ARR_QRING: n = h->sp[which - SIM_ARR_VIEW].tail * 32; break;
    case SIM_ARR_SLOTMAP: src = d.slot_of; n = (size_t)d.N * 4; break;
    default: return SIM_EINVAL;
  }
  *bytes = n;
  if (!buf) return SIM_OK;
  if (cap < n) return SIM_ERANGE;
  HCHECK(hipStreamSynchronize(h->stream));
  if (which == SIM_ARR_ROWS || which == SIM_ARR_QUEUE) {  // canonical form is assembled on the device
    DevScratch<uint8_t> tmp;
    if (int rc = tmp.alloc(n)) return rc;
    if (which == SIM_ARR_ROWS) canon_rows_kernel<<<grid_for(Nl), BLOCK, 0, h->stream>>>(d, (u64*)tmp.get());
    else canon_queue_kernel<<<grid_for(Nl), BLOCK, 0, h->stream>>>(d, (uint4*)tmp.get());
    // copy on the handle's stream: a non-blocking stream does not order against the null stream
    HCHECK(hipMemcpyAsync(buf, tmp.get(), n, hipMemcpyDeviceToHost, h->stream));
    HCHECK(hipStreamSynchronize(h->stream));
    return SIM_OK;
  }
  if (which >= SIM_ARR_VIEW && which <= SIM_ARR_QRING) return split_copy(h, h->sp[which - SIM_ARR_VIEW], buf, true);
  if (!src) { memset(buf, 0, n); return SIM_OK; }
  HCHECK(hipMemcpyAsync(buf, src, n, hipMemcpyDeviceToHost, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return SIM_OK;
}

// (LazyPlanes: the caller may ask about a Lamport time nobody has used yet — its ring plane gets memory, the bucket is empty)
static int conv_plane(sim_handle* h, u32 kind, u64 ltime) {
  if (kind != SIM_K_EVENT && kind != SIM_K_QUERY) return SIM_OK;
  SplitArr& A = h->sp[kind == SIM_K_EVENT ? SP_EV : SP_Q];
  return lazy_need(h, A.lz, (u64)h->d.X + ltime % (A.planes - h->d.X) + 1);  // (bucket t mod B is row X + t mod B)
}
// one pass of convergence_many_kernel: dev[0 .. cs.n] zeroed, counted into, copied to r[0 .. cs.n]; returns with the stream idle
static int conv_run(sim_handle* h, const ConvSet& cs, u64* dev, u64* r) {
  const size_t bytes = (size_t)(cs.n + 1) * 8;
  hipStream_t s = h->stream;
  HCHECK(hipMemsetAsync(dev, 0, bytes, s));
  convergence_many_kernel<<<grid_for(h->d.Nl), BLOCK, 0, s>>>(h->d, h->d_base, cs, dev);
  HCHECK(hipMemcpyAsync(r, dev, bytes, hipMemcpyDeviceToHost, s));
  HCHECK(hipStreamSynchronize(s));
  return SIM_OK;
}
int sim_convergence(sim_handle* h, uint32_t kind, uint32_t key, uint64_t ltime, uint64_t* seen, uint64_t* up) {
  if (!h || !seen || !up) return SIM_EINVAL;
  Dev& d = h->d;
  if (kind == SIM_K_JOIN || kind == SIM_K_LEAVE) { if (key >= d.N) return SIM_EINVAL; }
  else if (kind != SIM_K_EVENT && kind != SIM_K_QUERY) return SIM_EINVAL;
  if (int lrc = conv_plane(h, kind, ltime)) return lrc;
  ConvSet cs;
  memset(&cs, 0, sizeof cs);
  // key 0 of an EVENT / QUERY is "an empty place" of a bucket, no rumour: nobody holds it, the pass only counts the running nodes
  const bool nokey = !key && (kind == SIM_K_EVENT || kind == SIM_K_QUERY);
  cs.n = nokey ? 0 : 1; cs.kind[0] = kind; cs.key[0] = key; cs.ltime[0] = ltime;
  u64 r[2] = {0, 0};
  if (int rc = conv_run(h, cs, h->d_scratch + 8, r)) return rc;  // (the handle's own words: no allocation per call)
  *up = r[0];
  *seen = nokey ? 0 : r[1];
  return SIM_OK;
}

int sim_peek_packet(sim_handle* h, uint32_t node, uint32_t k, uint8_t* buf, size_t cap, size_t* len) {
  if (!h || !len || k >= h->d.f) return SIM_EINVAL;
  Dev& d = h->d;
  if (node < d.shard0 || node >= d.shard0 + d.Nl || h->in_tick) return SIM_EINVAL;
  namespace w = serf::wire;
  w::Bytes out;
  const TickP& p = h->prev;  // the map the packets in flight were sent with
  if (h->tick > 0 && k < p.feff) {
    u32 g = node / p.M, ll = node - g * p.M, hh, lp;
    fan_target_g(p, g, ll, k, hh, lp);
    std::vector<sim_packet> pages(d.PG);
    const uint4* src = (d.sharded && !d.rfan) ? d.xsend : cur_inbox(h);
    for (u32 pg = 0; pg < d.PG; ++pg) {
      size_t cell = d.rfan    ? (((size_t)k * d.PG + pg) * d.Nl + (node - d.shard0))  // random fan-out: the canonical inbox is sender-indexed
                    : d.sharded ? ((((size_t)((ll % p.blk) / p.sub) * p.V + hh) * d.fp + (size_t)k * d.PG + pg) * p.sub + lp % p.sub)
                              : (((size_t)k * d.PG + pg) * d.Nl + (size_t)hh * p.M + lp);
      HCHECK(hipMemcpyAsync(&pages[pg], src + cell * PK_U4, sizeof(sim_packet), hipMemcpyDeviceToHost, h->stream));
    }
    HCHECK(hipStreamSynchronize(h->stream));
    for (u32 pg = 0; pg < d.PG; ++pg)
      for (u32 r = 0; r < SIM_P; ++r) {
        const sim_packet& pk = pages[pg];
        u32 hm = pk.hi_meta[r], kind = (hm >> 4) & 15u, flags = hm & 15u;
        if (kind == SIM_K_EMPTY || kind >= SIM_K_ALIVE) continue;  // memberlist's own records are not serf messages
        u64 ltime = (u64)pk.val_lo[r] | ((u64)(hm >> 16) << 32);
        w::Bytes m;
        if (kind == SIM_K_JOIN) {
          w::Join j; j.ltime = ltime; j.id = pk.key[r];
          m = w::encode_message(j);
        } else if (kind == SIM_K_LEAVE) {
          w::Leave l; l.ltime = ltime; l.id = pk.key[r]; l.prune = flags & SIM_F_PRUNE;
          m = w::encode_message(l);
        } else if (kind == SIM_K_EVENT) {
          w::UserEvent e; e.ltime = ltime; e.cc = flags & SIM_F_CC;
          auto it = h->evreg.find(pk.key[r]);
          if (it != h->evreg.end()) { e.name = it->second.first; e.payload = it->second.second; }
          else { char nm[16]; int n = snprintf(nm, sizeof nm, "#%08x", pk.key[r]); e.name.assign(nm, nm + n); }
          m = w::encode_message(e);
        } else {
          w::Query q; q.ltime = ltime; q.id = pk.key[r];
          q.flags = ((flags & SIM_F_ACK) ? 1u : 0u) | ((flags & SIM_F_NO_BROADCAST) ? 2u : 0u);
          uint4 tj;
          HCHECK(hipMemcpy(&tj, d.qtab + pk.key[r] % SIM_QT, sizeof tj, hipMemcpyDeviceToHost));
          if (tj.x == pk.key[r]) { q.from_node = tj.y; q.relay_factor = (uint8_t)((tj.w >> 8) & 7u); }
          q.timeout_ms = (u64)h->q_timeout * 200u;  // gossip intervals of 200 ms
          q.name = {'#', 'q'};
          m = w::encode_message(q);
        }
        out.insert(out.end(), m.begin(), m.end());
      }
  }
  *len = out.size();
  if (!buf) return SIM_OK;
  if (out.size() > cap) return SIM_ERANGE;
  if (!out.empty()) memcpy(buf, out.data(), out.size());
  return SIM_OK;
}

int sim_convergence_many(sim_handle* h, uint32_t n, const uint32_t* kinds, const uint32_t* keys, const uint64_t* ltimes,
                         uint64_t* seen, uint64_t* up) {
  if (!h || !up || n > SIM_CONV_MAX || (n && (!kinds || !keys || !ltimes || !seen))) return SIM_EINVAL;
  Dev& d = h->d;
  ConvSet cs;
  memset(&cs, 0, sizeof cs);
  u32 at[SIM_CONV_MAX];  // the kernel's entry of rumour i; ~0: key 0 of an EVENT / QUERY, which nobody holds (sim_convergence)
  for (u32 i = 0; i < n; ++i) {
    if (kinds[i] == SIM_K_JOIN || kinds[i] == SIM_K_LEAVE) { if (keys[i] >= d.N) return SIM_EINVAL; }
    else if (kinds[i] != SIM_K_EVENT && kinds[i] != SIM_K_QUERY) return SIM_EINVAL;
    else if (!keys[i]) { at[i] = ~0u; continue; }
    at[i] = cs.n;
    cs.kind[cs.n] = kinds[i]; cs.key[cs.n] = keys[i]; cs.ltime[cs.n] = ltimes[i];
    cs.n++;
    if (int lrc = conv_plane(h, kinds[i], ltimes[i])) return lrc;
  }
  DevScratch<u64> scr;
  if (int rc = scr.alloc(SIM_CONV_MAX + 1)) return rc;
  u64 r[SIM_CONV_MAX + 1];
  if (int rc = conv_run(h, cs, scr.get(), r)) return rc;  // (returns with the stream idle)
  *up = r[0];
  for (u32 i = 0; i < n; ++i) seen[i] = at[i] == ~0u ? 0 : r[1 + at[i]];
  return SIM_OK;
}

// ---- checkpoint / resume (canonical image; layout documented in oracle/serf_oracle.c and DESIGN.md) ----
struct snap_header {
  uint32_t magic, abi;
  sim_config cfg;
  uint64_t tick;
  uint32_t n_slots, n_pending_ops;
  uint64_t ops_dropped, slots_recycled;
};
#define SNAP_MAGIC 0x53465253u
// the image's sections, in the order oracle/serf_oracle.c documents
enum { SEC_ROWS, SEC_QUEUE, SEC_INBOX, SEC_VIEW, SEC_ERING, SEC_QRING, SEC_SLOT_OF, SEC_SUBJECT_OF, SEC_BASE, SEC_UPMAP, SEC_QTAB, SEC_QBITS,
       SEC_OPS, SEC_ALLOC_TICK, SEC_QFILT, SEC_TAGS, SNAP_SECTIONS };
static_assert(SEC_VIEW + SP_Q == SEC_QRING && SEC_VIEW == (int)SIM_ARR_VIEW, "the split arrays' sections follow their descriptors");
// One section: its length and where it lives.  sim_snapshot takes it from the first of: a sim_dump_state array (`dump` >= 0: canonical
// form, assembled on the device), the handle's host copy, the device array.  sim_restore copies it to the device array (the dumped ones go
// back through their own kernels) and, last of all, to the host copy.
struct SnapSec {
  size_t len;
  int dump;
  void* host;
  void* dev;
};
static void snap_sections(sim_handle* h, size_t n_pending, SnapSec sec[SNAP_SECTIONS]) {
  const Dev& d = h->d;
  const size_t nup = ((size_t)d.N + 31) / 32;
  sec[SEC_ROWS] = {(size_t)d.Nl * sizeof(sim_row), SIM_ARR_ROWS, nullptr, nullptr};
  sec[SEC_QUEUE] = {(size_t)d.Nl * SIM_Q * sizeof(sim_record), SIM_ARR_QUEUE, nullptr, nullptr};
  sec[SEC_INBOX] = {(size_t)d.fp * d.Nl * sizeof(sim_packet), SIM_ARR_INBOX, nullptr, nullptr};
  for (int i = 0; i < SP_N; ++i) sec[SEC_VIEW + i] = {h->sp[i].tail * 32, SIM_ARR_VIEW + i, nullptr, nullptr};
  sec[SEC_SLOT_OF] = {(size_t)d.N * 4, -1, h->slot_of.data(), d.slot_of};
  sec[SEC_SUBJECT_OF] = {(size_t)d.A * 4, -1, h->subject_of.data(), d.subject_of};
  sec[SEC_BASE] = {(size_t)d.N * sizeof(sim_view), -1, h->base.data(), h->d_base};
  sec[SEC_UPMAP] = {nup * 4, -1, nullptr, d.upmap};
  sec[SEC_QTAB] = {(size_t)SIM_QT * 16, -1, nullptr, d.qtab};
  sec[SEC_QBITS] = {(size_t)SIM_QT * 2 * nup * 4, -1, nullptr, d.qbits};
  sec[SEC_OPS] = {n_pending * sizeof(OpEnt), -1, h->ops.data() + h->op_cursor, nullptr};  // (host only; restored through a vector of its own)
  sec[SEC_ALLOC_TICK] = {(size_t)d.A * 4, -1, h->alloc_tick.data(), nullptr};
  sec[SEC_QFILT] = {(size_t)SIM_QT * SIM_QF_WORDS * 4, -1, h->qfilt.data(), QFILT(d)};
  sec[SEC_TAGS] = {(size_t)d.N, -1, nullptr, TAGCLASS(d)};
}
int sim_snapshot(sim_handle* h, void* buf, size_t cap, size_t* bytes) {
  if (!h || !bytes) return SIM_EINVAL;
  if (h->in_tick) return SIM_ESTATE;  // between sim_step_begin and sim_step_end the state is half a tick ahead of `tick`
  Dev& d = h->d;
  if (d.swim && !d.sharded) {  // slot-less failed probes not yet replayed: into the schedule, so that the image holds them
    std::vector<u32> rq(2 * SIM_SUSPECT_REQ_MAX);
    for (u64 back = 2; back >= 1; --back) {
      if (h->tick < back) continue;
      u32 n = 0;
      int rc = sreq_take(h, h->tick - back, rq.data(), SIM_SUSPECT_REQ_MAX, &n);
      if (rc) return rc;
      for (u32 i = 0; i < n; ++i)
        if ((rc = inject_val(h, h->tick + 2 - back, SIM_OP_SUSPECT, rq[2 * i], rq[2 * i + 1], 0, 0)) != SIM_OK) return rc;
    }
  }
  SnapSec sec[SNAP_SECTIONS];
  snap_sections(h, h->ops.size() - h->op_cursor, sec);
  size_t tot = sizeof(snap_header);
  for (const SnapSec& sc : sec) tot += 8 + sc.len;
  *bytes = tot;
  if (!buf) return SIM_OK;
  if (cap < tot) return SIM_ERANGE;
  HCHECK(hipStreamSynchronize(h->stream));
  snap_header hd;
  memset(&hd, 0, sizeof hd);
  hd.magic = SNAP_MAGIC; hd.abi = SIM_ABI_VERSION; hd.cfg = h->cfg; hd.tick = h->tick; hd.n_slots = h->n_slots;
  hd.n_pending_ops = (uint32_t)(h->ops.size() - h->op_cursor);
  hd.ops_dropped = h->ops_dropped; hd.slots_recycled = h->slots_recycled;
  uint8_t* o = (uint8_t*)buf;
  memcpy(o, &hd, sizeof hd); o += sizeof hd;
  for (const SnapSec& sc : sec) {
    const uint64_t n = sc.len;
    memcpy(o, &n, 8); o += 8;
    if (sc.dump >= 0) {
      size_t got = 0;
      if (int rc = sim_dump_state(h, (uint32_t)sc.dump, o, n, &got)) return rc;
    } else if (sc.host) {
      if (n) memcpy(o, sc.host, n);
    } else {
      HCHECK(hipMemcpyAsync(o, sc.dev, n, hipMemcpyDeviceToHost, h->stream));
      HCHECK(hipStreamSynchronize(h->stream));
    }
    o += n;
  }
  return SIM_OK;
}
int sim_restore(sim_handle* h, const void* buf, size_t bytes) {
  if (!h || !buf || bytes < sizeof(snap_header)) return SIM_EINVAL;
  if (h->tick != 0 || !h->ops.empty()) return SIM_ESTATE;
  Dev& d = h->d;
  snap_header hd;
  memcpy(&hd, buf, sizeof hd);
  if (hd.magic != SNAP_MAGIC || hd.abi != SIM_ABI_VERSION || memcmp(&hd.cfg, &h->cfg, sizeof(sim_config))) return SIM_EINVAL;
  // ---- pass 1: validate the header, every section length and what the kernels index with, before anything is touched ----
  if (hd.tick > SIM_TICK_MAX) return SIM_EINVAL;                    // a handle executes no tick beyond it (include/serf_sim.h)
  if (hd.n_slots > d.A) return SIM_EINVAL;                          // reap_run / pp_merge walk a < n_slots
  if ((size_t)hd.n_pending_ops > bytes / sizeof(OpEnt)) return SIM_EINVAL;  // sizes a host allocation
  SnapSec sec[SNAP_SECTIONS];
  snap_sections(h, hd.n_pending_ops, sec);
  const uint8_t* img[SNAP_SECTIONS];
  {
    const uint8_t* in = (const uint8_t*)buf + sizeof hd;
    const uint8_t* end = (const uint8_t*)buf + bytes;
    for (int i = 0; i < SNAP_SECTIONS; ++i) {
      uint64_t n;
      if ((size_t)(end - in) < 8) return SIM_EINVAL;
      memcpy(&n, in, 8); in += 8;
      if (n != sec[i].len || (size_t)(end - in) < n) return SIM_EINVAL;
      img[i] = in;
      in += n;
    }
  }
  uint4* inbox_dst = (d.sharded && !d.rfan) ? h->rbuf[(hd.tick + 1) & 1] : h->inbox_mat;
  if ((sec[SEC_INBOX].len && !inbox_dst) || (d.sharded && d.rfan && !h->bound)) return SIM_ESTATE;  // sharded: bind the exchange buffers first
  {  // slot maps must be consistent with n_slots (they index the view) and with each other (the recycling scan and
     // ensure_slot go from a slot to its subject and back)
    const u32* so = (const u32*)img[SEC_SLOT_OF];
    const u32* sj = (const u32*)img[SEC_SUBJECT_OF];
    for (u32 i = 0; i < d.N; ++i)
      if (so[i] != NOSLOT && (so[i] >= (h->dense ? d.A : hd.n_slots) || sj[so[i]] != i)) return SIM_EINVAL;
    for (u32 a = 0; a < d.A; ++a)
      if (sj[a] != NOSLOT && (sj[a] >= d.N || so[sj[a]] != a)) return SIM_EINVAL;
  }
  // the pending schedule goes straight to ops_kernel: the same checks sim_inject applies (parsed into a vector of its own)
  std::vector<OpEnt> new_ops(hd.n_pending_ops, OpEnt{0, 0, 0, 0, 0});
  if (sec[SEC_OPS].len) memcpy(new_ops.data(), img[SEC_OPS], sec[SEC_OPS].len);
  for (const OpEnt& e : new_ops)
    if (op_validate(d.N, e.op, e.node, e.a, e.b) != SIM_OK) return SIM_EINVAL;
  for (u32 j = 0; j < SIM_QT; ++j)  // the kernel loops over n_ids and shifts by the class
    if (((const u32*)img[SEC_QFILT])[(size_t)j * SIM_QF_WORDS + 1] > SIM_QF_IDS) return SIM_EINVAL;
  for (u32 i = 0; i < d.N; ++i)
    if (img[SEC_TAGS][i] >= SIM_TAG_CLASSES) return SIM_EINVAL;
  // ---- pass 2: everything that can fail for lack of memory, before the first byte of the image reaches the device (ADVICE r5, r6) ----
  hipStream_t s = h->stream;
  DevScratch<uint8_t> tmp_rows, tmp_queue;
  if (int rc = tmp_rows.alloc(sec[SEC_ROWS].len)) return rc;
  if (int rc = tmp_queue.alloc(sec[SEC_QUEUE].len)) return rc;
  {
    // LazyPlanes: memory for the planes the image has anything in (what is mapped beyond them is overwritten with the image's zeros) and
    // for the planes that need it whatever the image holds — a slot that was handed out may hold nothing but zeros
    u64 need[SP_N] = {hd.n_slots, 0, 0};
    for (int i = 0; i < SP_N; ++i) {
      if (!h->sp[i].lz.va) continue;
      const size_t pb = (size_t)d.Nl * 32;
      u32 used = h->sp[i].planes;
      while (used > 0) {  // the last plane with a non-zero byte
        const uint8_t* p = img[SEC_VIEW + i] + (size_t)(used - 1) * pb;
        if (p[0] || memcmp(p, p + 1, pb - 1)) break;
        --used;
      }
      need[i] = std::max<u64>(need[i], used);
    }
    // ... and the bounds on the clocks from the image — the rows' clocks, what the pending operations add — with the ring planes they need
    u64 eh = 1, qh = 1;
    if (h->sp[SP_EV].lz.va || h->sp[SP_Q].lz.va) {
      for (size_t i = 0; i < d.Nl; ++i) {
        sim_row r;
        memcpy(&r, img[SEC_ROWS] + i * sizeof(sim_row), sizeof r);
        eh = std::max(eh, r.event_clock); qh = std::max(qh, r.query_clock);
      }
      for (const OpEnt& e : new_ops) {
        const u64 t1 = std::min<u64>(e.val, ~0ull - 4) + 1;
        if (e.op == SIM_OP_USER_EVENT) ++eh;
        else if (e.op == SIM_OP_QUERY) ++qh;
        else if ((e.op == SIM_OP_DELIVER && SIM_META_KIND(e.b) == SIM_K_EVENT) || (e.op == SIM_OP_WITNESS && e.a == 1u)) eh = std::max(eh, t1);
        else if ((e.op == SIM_OP_DELIVER && SIM_META_KIND(e.b) == SIM_K_QUERY) || (e.op == SIM_OP_WITNESS && e.a == 2u)) qh = std::max(qh, t1);
      }
      // (a pending event originates at a clock <= the maximum so far; its witnesses end one above it)
    }
    const u64 eh0 = h->ev_hi, qh0 = h->q_hi;
    h->ev_hi = std::max(eh, eh0); h->q_hi = std::max(qh, qh0);
    int lrc = SIM_OK;
    for (int i = 0; i < SP_N && lrc == SIM_OK; ++i) lrc = lazy_need(h, h->sp[i].lz, need[i]);
    if (lrc == SIM_OK) lrc = rings_need(h);
    if (lrc) { h->ev_hi = eh0; h->q_hi = qh0; return lrc; }  // the handle is still the fresh one it was (with some planes more, all zeros)
  }
  // ---- pass 3: device copies, behind the planes' memsets (the handle's host state is committed only after they succeed) ----
  auto up = [&](void* dst, int i) { return sec[i].len ? hipMemcpyAsync(dst, img[i], sec[i].len, hipMemcpyHostToDevice, s) : hipSuccess; };
  HCHECK(up(tmp_rows.get(), SEC_ROWS)); HCHECK(up(tmp_queue.get(), SEC_QUEUE)); HCHECK(up(inbox_dst, SEC_INBOX));
  for (int i = 0; i < SP_N; ++i)
    if (int rc = split_copy(h, h->sp[i], (void*)img[SEC_VIEW + i], false)) return rc;
  for (int i = SEC_SLOT_OF; i < SNAP_SECTIONS; ++i)
    if (sec[i].dev) HCHECK(up(sec[i].dev, i));
  // canonical rows / queue -> packed row groups, sort keys + slot-stable payloads
  HCHECK(hipMemsetAsync(d.R2, 0, (size_t)d.Nl * 16, s));
  restore_queue_kernel<<<grid_for(d.Nl), BLOCK, 0, s>>>(d, (const uint4*)tmp_queue.get());
  restore_rows_kernel<<<grid_for(d.Nl), BLOCK, 0, s>>>(d, (const u64*)tmp_rows.get());
  if (!d.sharded || d.rfan) {  // the packets in flight go back to their senders (one cell per slot)
    TickP p;
    tickp_make(&p, &h->cfg, hd.tick ? hd.tick - 1 : 0);
    // (random fan-out: the graph of the packets in flight is a function of (seed, tick - 1): sim_step_begin builds it again)
    unmaterialize_kernel<<<grid_for(d.Nl), BLOCK, 0, s>>>(d, p, (u32)(hd.tick & 1), hd.tick ? 1u : 0u, h->inbox_mat);
  }
  HCHECK(hipGetLastError());
  HCHECK(hipStreamSynchronize(s));  // (the scratch goes after this)
  // ---- the host state ----
  h->tick = hd.tick;
  h->mat_tick = (d.sharded && !d.rfan) ? ~0ull : hd.tick;  // the image's inbox section is what sits in inbox_mat
  h->n_slots = hd.n_slots;
  if (hd.tick > 0) tickp_make(&h->prev, &h->cfg, hd.tick - 1);  // the parameters the packets in flight were sent with
  memcpy(h->slot_of.data(), img[SEC_SLOT_OF], sec[SEC_SLOT_OF].len);
  memcpy(h->subject_of.data(), img[SEC_SUBJECT_OF], sec[SEC_SUBJECT_OF].len);
  memcpy(h->base.data(), img[SEC_BASE], sec[SEC_BASE].len);
  h->walk.clear();
  for (u32 subj = 0; subj < d.N; ++subj)
    if (h->slot_of[subj] != NOSLOT) h->walk.push_back(h->slot_of[subj]);
  if (!h->walk.empty()) HCHECK(hipMemcpy(d.walk, h->walk.data(), h->walk.size() * 4, hipMemcpyHostToDevice));
  h->ops.swap(new_ops);
  memcpy(h->alloc_tick.data(), img[SEC_ALLOC_TICK], sec[SEC_ALLOC_TICK].len);
  memcpy(h->qfilt.data(), img[SEC_QFILT], sec[SEC_QFILT].len);
  h->n_alloc = (u32)h->walk.size();
  h->ops_dropped = hd.ops_dropped; h->slots_recycled = hd.slots_recycled;
  h->recycle_at = 0xFFFFFFFFu;
  h->pp_done_at = 0xFFFFFFFFu;
  h->op_cursor = 0;
  if (int rc = rf_reset(h)) return rc;
  if (h->xflag) *h->xflag = 0;
  if (d.sharded && d.rfan && hd.tick > 0) {
    // the packets in flight are back in their senders' cells: packed again — the host runs the round's exchange once more
    // before the next tick (SIM_XCHG_PACKED)
    for (u32 c = 0; c < h->rf_C; ++c) {
      int prc = rfx_pack(h, hd.tick - 1, c);
      if (prc) return prc;
    }
    HCHECK(hipStreamSynchronize(h->stream));
  }
  return SIM_OK;
}
int sim_query_status(sim_handle* h, uint32_t qid, uint64_t* acks, uint64_t* responses, int* open) {
  if (!h || !acks || !responses || !open || !qid) return SIM_EINVAL;
  Dev& d = h->d;
  hipStream_t s = h->stream;
  u32 j = qid % SIM_QT;
  uint4 tj;
  HCHECK(hipMemcpyAsync(&tj, d.qtab + j, sizeof tj, hipMemcpyDeviceToHost, s));
  HCHECK(hipStreamSynchronize(s));
  if (tj.x != qid) return SIM_EINVAL;
  size_t words = ((size_t)d.N + 31) / 32;
  HCHECK(hipMemsetAsync(h->d_scratch + 10, 0, 16, s));
  query_count_kernel<<<grid_for(words), BLOCK, 0, s>>>(d.qbits + (size_t)j * 2 * words, words, h->d_scratch + 10);
  u64 r[2];
  HCHECK(hipMemcpyAsync(r, h->d_scratch + 10, 16, hipMemcpyDeviceToHost, s));
  HCHECK(hipStreamSynchronize(s));
  *acks = r[0];
  *responses = r[1];
  *open = (u32)h->tick <= tj.z;
  return SIM_OK;
}
int sim_query_responders(sim_handle* h, uint32_t qid, int which, uint32_t* out, uint32_t cap, uint32_t* n) {
  if (!h || !n || !qid || (which != 0 && which != 1) || (cap && !out)) return SIM_EINVAL;
  Dev& d = h->d;
  hipStream_t s = h->stream;
  u32 j = qid % SIM_QT;
  uint4 tj;
  HCHECK(hipMemcpyAsync(&tj, d.qtab + j, sizeof tj, hipMemcpyDeviceToHost, s));
  HCHECK(hipStreamSynchronize(s));
  if (tj.x != qid) return SIM_EINVAL;
  size_t words = ((size_t)d.N + 31) / 32;
  std::vector<u32> bits(words);  // one bit per node: the bitmap itself is the compact form (128 KiB at 1 Mi nodes)
  HCHECK(hipMemcpyAsync(bits.data(), d.qbits + ((size_t)j * 2 + (size_t)which) * words, words * 4, hipMemcpyDeviceToHost, s));
  HCHECK(hipStreamSynchronize(s));
  u32 k = 0;
  for (u32 g = d.shard0; g < d.shard0 + d.Nl; ++g)
    if ((bits[g >> 5] >> (g & 31)) & 1u) { if (k < cap) out[k] = g; ++k; }
  *n = k;
  return SIM_OK;
}
int sim_profile(sim_handle* h, int enable) {
  if (!h) return SIM_EINVAL;
  h->profiling = enable > 0 ? (u32)enable : 0u;
  h->prof_seq = 0;
  return SIM_OK;
}
int sim_profile_read_stats(sim_handle* h, double out_ms[3], uint64_t* launches) {
  if (!h || !out_ms || !launches) return SIM_EINVAL;
  HCHECK(hipStreamSynchronize(h->stream));
  double tot = 0.0, mn = 0.0, mx = 0.0;
  bool first = true;
  for (auto& pr : h->prof) {
    float t = 0.f;
    HCHECK(hipEventElapsedTime(&t, pr.first, pr.second));
    tot += t;
    mn = first ? t : std::min<double>(mn, t);
    mx = first ? t : std::max<double>(mx, t);
    first = false;
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  out_ms[0] = tot; out_ms[1] = mn; out_ms[2] = mx;
  *launches = h->prof.size();
  for (int i = 0; i < 3; ++i) h->sreq_wait[i] = nullptr;  // (the stream was synchronised above: every tick has finished)
  h->prof.clear();
  return SIM_OK;
}
int sim_profile_read(sim_handle* h, double* ms, uint64_t* launches) {  // the total alone
  if (!ms) return SIM_EINVAL;
  double out_ms[3];
  const int rc = sim_profile_read_stats(h, out_ms, launches);
  if (rc == SIM_OK) *ms = out_ms[0];
  return rc;
}
int sim_resident_planes(const sim_handle* h, uint32_t out[6], uint64_t* bytes_per_plane) {
  if (!h || !out) return SIM_EINVAL;
  for (int i = 0; i < SP_N; ++i) { out[2 * i] = split_mapped(h->sp[i]); out[2 * i + 1] = h->sp[i].planes; }
  if (bytes_per_plane) *bytes_per_plane = (uint64_t)h->d.Nl * 32;
  return SIM_OK;
}
int sim_cluster_stats_get(sim_handle* h, sim_cluster_stats* out) {
  if (!h || !out) return SIM_EINVAL;
  Dev& d = h->d;
  hipStream_t s = h->stream;
  DevScratch<u64> scr;  // [10] the figures, then [workgroups][10] partial ones
  const u32 nwg = (u32)std::min<int>(grid_for(d.Nl), CSTAT_WG);
  if (int rc = scr.alloc((size_t)(1 + nwg) * 10)) return rc;
  u64 r[10];
  // sharded: the packets in flight sit in the receive buffer, [src][k][blk] = f * Nl cells as well
  cluster_stats_kernel<<<nwg, BLOCK, 0, s>>>(d, cur_inbox(h), scr.get() + 10);
  cluster_stats_fold<<<1, dim3(64, 10), 0, s>>>(scr.get() + 10, nwg, scr.get());
  HCHECK(hipMemcpyAsync(r, scr.get(), sizeof r, hipMemcpyDeviceToHost, s));
  u32 evc = 0;
  HCHECK(hipMemcpyAsync(&evc, d.ev_count, 4, hipMemcpyDeviceToHost, s));
  HCHECK(hipStreamSynchronize(s));
  out->up = r[0];
  for (int i = 0; i < 4; ++i) out->queued[i] = r[1 + i];
  out->overflow = r[5]; out->inbox_records = r[6]; out->failed = r[7]; out->left = r[8]; out->max_queue = r[9];
  out->ops_dropped = h->ops_dropped; out->slots_in_use = h->n_alloc; out->slots_recycled = h->slots_recycled;
  out->events_lost = h->events_lost + (evc > d.ev_cap ? evc - d.ev_cap : 0);
  return SIM_OK;
}
