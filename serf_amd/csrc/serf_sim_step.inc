// serf_sim_step.inc — part of the translation unit serf_sim.hip (included from there, behind the extern "C" block of the API; not a header of its own).
// host: what runs every tick.  Host statics first, with C++ linkage (templates), then the entry points in an extern "C" block of their own;
// what the rest of the library needs from here is declared in serf_sim_host.inc.
// One launch: with events on its dispatch when it is given a stop event, plain otherwise; every argument is cast to the kernel's parameter type.
template <typename... KA, typename... A>
static void launch_ev(void (*k)(KA...), int grid, int block, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const A&... a) {
  if (e1) hipExtLaunchKernelGGL(k, dim3(grid), dim3(block), 0, s, e0, e1, 0, static_cast<KA>(a)...);
  else hipLaunchKernelGGL(k, dim3(grid), dim3(block), 0, s, static_cast<KA>(a)...);
}
// The event that marks "tick t's kernel has finished" (the tick in progress once its last launch is enqueued, or one of the two before
// it), or null: sreq_ev[t % 3] — recorded behind the launch by sim_step_end, or riding on the dispatch of the tick's one launch / last
// pack as its stop event — or the stop event of the tick's timing pair.  Null: SWIM is off, or sim_profile_read_stats has run since: it
// nulls all three, because one may be a timing event it has just destroyed (it synchronises the stream first: nobody needs to wait).
static hipEvent_t tick_done_event(const sim_handle* h, u64 t) { return h->sreq_wait[t % 3]; }
// ---- the fan-out graph as a CSR, rebuilt every tick (SIM_CF_RANDOM_FANOUT); its schedule: sim_handle::rf_q, serf_sim_host.inc ----
template <typename E>
static bool rf_attrs(const RfP& r) {
  const int rl = (int)rf_rows_lds(r);
  return hipFuncSetAttribute(reinterpret_cast<const void*>(rf_rows_kernel<E, RF_EPT, (1u << RF_LB_MAX) / RFR>), hipFuncAttributeMaxDynamicSharedMemorySize, rl) == hipSuccess &&
         hipFuncSetAttribute(reinterpret_cast<const void*>(rf_rows_kernel<E, 11u, 2u>), hipFuncAttributeMaxDynamicSharedMemorySize, rl) == hipSuccess &&
         hipFuncSetAttribute(reinterpret_cast<const void*>(rf_scatter_kernel<E>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rf_scatter_lds<E>(r)) == hipSuccess;
}
// its parameters, scratch, stream and events
static int create_rf(sim_handle* h) {
  const sim_config* cfg = &h->cfg;
  Dev& d = h->d;
  const size_t Nl = d.Nl;
  RfP& r = h->rfp;
  r.N = d.N; r.Nl = d.Nl; r.shard0 = d.shard0; r.f = d.f;
  r.Ns = d.Nl;  // every handle sorts the pairs of its OWN senders: by (local) target — or, a shard, by target anywhere in the cluster
  r.V = d.sharded ? d.V : 1u; r.M = d.sharded ? d.M : d.N;
  if (d.sharded && d.V > 64u) return SIM_EINVAL;
  // the sorted list: every pair of the handle's senders, f * Nl at most.  The rows a shard RECEIVES (rx_rsrc): f * Nl on average
  const size_t np = (size_t)d.f * Nl, nrx = (size_t)d.f * Nl + (size_t)(12.0 * std::sqrt((double)d.f * Nl)) + 4096u;
  r.rcap = (u32)np;
  // level-1 buckets of 2^LB targets.  A scattered entry carries the pair id (PB bits) and the target's offset in its bucket
  // (LB bits) — rf_rows does not draw again —; 32-bit entries when both fit (1 Mi nodes: 22 + 10), 64-bit ones otherwise.
  // A shard's buckets are per destination (V * ceil(M / 2^LB) of them): narrow entries while that keeps rf_scatter's three
  // tables in 48 KiB of LDS, else wide ones and about 2048 buckets
  r.PB = 1;
  while ((1ull << r.PB) < 4ull * r.Ns) r.PB++;
  auto nb_of = [&](u32 lb) { return (size_t)r.V * (((size_t)r.M + (1u << lb) - 1u) >> lb); };
  r.LB = std::min<u32>(11u, 32u - std::min<u32>(r.PB, 24u));
  if (const char* e = getenv("SERF_RF_LB")) r.LB = std::min<u32>(RF_LB_MAX, std::max<u32>(8u, (u32)strtoul(e, nullptr, 0)));
  while (nb_of(r.LB) > (r.V > 1u && r.PB + r.LB > 32u ? 2048u : 4096u) && r.LB < RF_LB_MAX) r.LB++;  // rf_scatter's three tables: 48 KiB of LDS next to its staging area
  if (nb_of(r.LB) > 4096u) return SIM_EINVAL;
  h->rf_wide = r.PB + r.LB > 32u || getenv("SERF_RF_WIDE") != nullptr;
  r.NBh = (u32)(nb_of(r.LB) / r.V);
  r.NB = r.V * r.NBh;
  r.NWG = (u32)(((size_t)r.Ns + (h->rf_wide ? RfSpw<u64>::v : RfSpw<u32>::v) - 1u) / (h->rf_wide ? RfSpw<u64>::v : RfSpw<u32>::v));
  // pairs of a bucket: f per row on one handle; a shard's f * M pairs spread over all V * NBh buckets
  const double mean = (double)d.f * (double)(1u << r.LB) / (double)r.V;
  r.cap = std::min<u32>(std::max<u32>(((u32)(mean + 16.0 * std::sqrt(mean)) + 64u + RFR - 1u) / RFR * RFR, RFR), RF_EPT * RFR);  // 16 sigma and more of room
  if (r.V == 1u) r.cap = std::min<u32>(6u << r.LB, std::max<u32>(r.cap, RFR));  // one handle: mean f * 2^LB and 16 sigma, rounded up to the workgroup (5 632 at 1 Mi nodes: 11 pairs per thread)
  if (const char* e = getenv("SERF_RF_CAP")) r.cap = std::max<u32>(RFR, std::min<u32>(r.cap, (u32)strtoul(e, nullptr, 0)) / RFR * RFR);  // tests: force rf_rows' slow path
  // a bucket's region of l1: the mean and 12 sigma; what does not fit goes onto the overflow list
  r.bcap = (u32)(mean + 12.0 * std::sqrt(mean)) + 64u;
  if (const char* e = getenv("SERF_RF_BCAP")) r.bcap = std::max<u32>(1u, (u32)strtoul(e, nullptr, 0));  // tests: force the overflow list
  r.ocap = (u32)np;  // (every pair would fit: the list cannot run full)
  if (!(h->rf_wide ? rf_attrs<u64>(r) : rf_attrs<u32>(r))) return SIM_EDEVICE;
  if (hipHostMalloc((void**)&h->xflag, 64) != hipSuccess) return SIM_ENOMEM;
  *h->xflag = 0;
  if (d.sharded) {
    h->rf_C = cfg->chunks > 1 ? cfg->chunks : 1u;  // sender chunks: each packed and exchanged behind its own launch
    h->rfx = rfx_layout(d.V, h->rf_C, d.M, r.NBh, r.LB, d.PG, d.f);
    if ((size_t)h->rf_C * d.V * h->rfx.slab_u >= ((size_t)1 << 30) ||   // rfx_index_kernel's 32-bit cell index: the receive buffer holds C * V slabs (ADVICE r5)
        hipFuncSetAttribute(reinterpret_cast<const void*>(rfx_index_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rfx_index_lds(h->rfx)) != hipSuccess) return SIM_EINVAL;
    for (int i = 0; i < 3; ++i) { DA(h->rf_cntb[i], (size_t)d.N * h->rf_C) DA(h->rf_btot[i], (size_t)r.NB * h->rf_C) DA(h->rf_xoff[i], (2 * (size_t)d.V + 2) * h->rf_C) }
    DA(h->rx_rcsr, Nl + 1) DA(h->rx_rsrc, nrx)
    if (hipMemset(h->rx_rcsr, 0, (Nl + 1) * 4) != hipSuccess) return SIM_EDEVICE;  // tick 0 receives nothing
  }
  h->rf_sync = getenv("SERF_RF_SYNC") != nullptr;  // measurements: build on the tick's own stream, nothing overlaps
  for (int i = 0; i < 3; ++i) { DA(h->rf_rcsr[i], Nl + 1) DA(h->rf_rsrc[i], np) }
  h->rx_cap = (u32)nrx;
  const size_t esz = h->rf_wide ? 2 : 1;  // (in u32 words)
  u32* p32 = nullptr;
  for (int i = 0; i < 2; ++i) { DA(h->rf_gcur[i], (size_t)r.NB * RF_GCS) DA(p32, (1 + 2 * (size_t)r.ocap) * esz) h->rf_ovf[i] = p32; }
  DA(p32, (size_t)r.NB * r.bcap * esz)
  h->rf_l1 = p32;
  bool ok = true;
  for (int i = 0; i < 3; ++i) ok = ok && hipMemset(h->rf_rcsr[i], 0, (Nl + 1) * 4) == hipSuccess;  // tick 0 receives nothing
  for (int i = 0; i < 2; ++i) ok = ok && hipMemset(h->rf_gcur[i], 0, (size_t)r.NB * RF_GCS * 4) == hipSuccess && hipMemset(h->rf_ovf[i], 0, 8) == hipSuccess;
  {  // the build stream; SERF_RF_PRIO=high|low: at the highest / lowest stream priority (measurements)
    int plo = 0, phi = 0;
    const char* pe = getenv("SERF_RF_PRIO");
    // (r6) a shard: at the highest priority — a priority level has hardware queues of its own, and a process that also holds an
    // exchange stream, torch's streams and RCCL's found the build sharing the handle's queue: every build ran between two tick
    // kernels instead of beside one (profiles/r06_experiments.md §7)
    if (!pe && d.sharded) pe = "high";
    if (pe && *pe != 'n' && hipDeviceGetStreamPriorityRange(&plo, &phi) == hipSuccess)
      ok = ok && hipStreamCreateWithPriority(&h->rf_stream, hipStreamNonBlocking, *pe == 'h' ? phi : plo) == hipSuccess;
    else ok = ok && hipStreamCreateWithFlags(&h->rf_stream, hipStreamNonBlocking) == hipSuccess;
  }
  for (hipEvent_t* e : {&h->rf_done[0], &h->rf_done[1], &h->rf_done[2], &h->rf_go[0], &h->rf_go[1]})
    ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
  return ok ? SIM_OK : SIM_EDEVICE;
}
static bool rf_lean(const RfP& r) { return r.cap <= 11u * RFR && (1u << r.LB) <= 2u * RFR; }  // rf_rows' lean instantiation: 11 pairs and 2 rows per thread are enough
// the fan-out graph of `tick`, on stream `s`: rf_rcsr / rf_rsrc [tick % 3] := the rows of the packets sent during `tick` (E: the entry type)
template <typename E>
static int rf_build_as(sim_handle* h, u64 tick, hipStream_t s) {
  RfP r = h->rfp;
  TickP tp;
  tickp_make(&tp, &h->cfg, tick);
  r.rb = rng_base(h->cfg.seed, STREAM_RFAN, tick);
  r.feff = tp.feff;
  // a shard sorts the pairs of every sender chunk on their own (SIM_XCHG_PACKED: chunk c's slabs leave behind chunk c's launch)
  const u32 C = h->d.sharded ? h->rf_C : 1u;
  r.Ns = h->d.Nl / C;
  r.rcap = h->d.f * r.Ns;
  r.NWG = (u32)(((size_t)r.Ns + RfSpw<E>::v - 1u) / RfSpw<E>::v);
  const bool lean = rf_lean(r);
  for (u32 c = 0; c < C; ++c) {
    r.lfirst = c * r.Ns;
    u32 *rcsr = h->rf_rcsr[tick % 3], *rsrc = h->rf_rsrc[tick % 3] + (size_t)c * r.rcap;
    uint8_t* cntb = h->d.sharded ? h->rf_cntb[tick % 3] + (size_t)c * h->d.N : nullptr;  // a shard: the sending side's sort
    u32* btot = h->d.sharded ? h->rf_btot[tick % 3] + (size_t)c * r.NB : nullptr;
    const u32 par = h->rf_par;
    h->rf_par ^= 1u;
    u32 *g = h->rf_gcur[par], *gn = h->rf_gcur[par ^ 1u];
    E *l1 = (E*)h->rf_l1, *ovf = (E*)h->rf_ovf[par], *ovfn = (E*)h->rf_ovf[par ^ 1u];
    rf_scatter_kernel<E><<<r.NWG, RFB, rf_scatter_lds<E>(r), s>>>(r, g, l1, ovf);
    if (lean) rf_rows_kernel<E, 11u, 2u><<<r.NB, RFR, rf_rows_lds(r), s>>>(r, g, gn, (const E*)l1, ovf, ovfn, rcsr, rsrc, cntb, btot, h->xflag);
    else rf_rows_kernel<E, RF_EPT, (1u << RF_LB_MAX) / RFR><<<r.NB, RFR, rf_rows_lds(r), s>>>(r, g, gn, (const E*)l1, ovf, ovfn, rcsr, rsrc, cntb, btot, h->xflag);
    if (h->d.sharded) rfx_soff_kernel<<<1, 256, 0, s>>>(h->rfx, btot, h->rf_xoff[tick % 3] + (size_t)c * (2u * h->d.V + 2u), h->xflag);
  }
  HCHECK(hipGetLastError());
  return SIM_OK;
}
static int rf_build(sim_handle* h, u64 tick, hipStream_t s) { return h->rf_wide ? rf_build_as<u64>(h, tick, s) : rf_build_as<u32>(h, tick, s); }
// The graph of tick s stands before whatever is enqueued on the handle's stream next.  It was enqueued on the build stream two ticks
// ago (a shard's: a tick ago); right after a restore, at tick 1, or with SERF_RF_SYNC nobody queued it: it is built here and now.
// Otherwise the stream waits for the build — unless the host can see that it has finished, as it has in the steady state: a wait that
// is already over is still a barrier packet between two tick kernels, or between the launch and the pack.
static int rf_ready(sim_handle* h, u64 s) {
  const u32 i = (u32)(s % 3);
  if (h->rf_q[i] != s) {
    int rc = rf_build(h, s, h->stream);
    if (rc) return rc;
    h->rf_q[i] = s;
  } else if (hipEventQuery(h->rf_done[i]) != hipSuccess) HCHECK(hipStreamWaitEvent(h->stream, h->rf_done[i], 0));
  return SIM_OK;
}
// The look-ahead, when tick h->tick begins: the graphs of THIS tick's packets and the next tick's are enqueued on the build stream if
// they are not yet — as soon as everything enqueued so far has finished: they overwrite a buffer the tick before this one read.
static int rf_look_ahead(sim_handle* h) {
  bool waited = false;
  // (a shard needs the sort of tick t as soon as tick t has computed — the pack —, a tick earlier than a handle that holds every
  // node needs its rows: one build further ahead; the third buffer is free — the pack of tick t - 1 was its last reader)
  for (u64 s = h->tick; s <= h->tick + (h->d.sharded ? 2u : 1u); ++s) {
    if (h->rf_q[s % 3] == s) continue;
    if (!waited) {
      // the one go signal of this call: the builds wait for the kernel of the tick before — for the stop event its dispatch carries,
      // while its request list is unread (no marker packet of our own in the handle's stream), else for a marker
      hipEvent_t prev = h->tick > 0 ? tick_done_event(h, h->tick - 1) : nullptr;
      if (prev && h->sreq_tick[(h->tick - 1) % 3] == h->tick - 1) HCHECK(hipStreamWaitEvent(h->rf_stream, prev, 0));
      else {
        hipEvent_t go = h->rf_go[h->tick & 1];
        HCHECK(hipEventRecord(go, h->stream));
        HCHECK(hipStreamWaitEvent(h->rf_stream, go, 0));
      }
      waited = true;
    }
    int rc = rf_build(h, s, h->rf_stream);
    if (rc) return rc;
    HCHECK(hipEventRecord(h->rf_done[s % 3], h->rf_stream));
    h->rf_q[s % 3] = s;
  }
  return SIM_OK;
}
// no graph is queued (sim_restore); a build of the run that is being replaced may still be writing the scratch
static int rf_reset(sim_handle* h) {
  if (h->rf_stream) HCHECK(hipStreamSynchronize(h->rf_stream));
  for (int i = 0; i < 3; ++i) h->rf_q[i] = ~0ull;
  return SIM_OK;
}
// random fan-out on a shard: the packets sent during tick `t` (in their senders' cells) -> the V slabs of the send buffer, on the
// handle's stream, behind the tick's launch (SIM_XCHG_PACKED).
static int rfx_pack(sim_handle* h, u64 t, u32 c /* sender chunk */) {
  Dev& d = h->d;
  // (r6, tried: the pack on the exchange stream, beside the launch of the next sender chunk — every hop between two streams costs
  // 30 - 50 us of latency on this platform, more than the overlap hides: profiles/r06_experiments.md §7)
  if (int rc = rf_ready(h, t)) return rc;
  const RfxL& x = h->rfx;
  const u32 per = d.f * (d.Nl / x.C);   // pairs of one chunk
  const u32* xoff = h->rf_xoff[t % 3] + (size_t)c * (2u * x.V + 2u);
  uint4* send = d.xsend + (size_t)c * x.V * x.slab_u * 4u;   // slab (c, 0)
  // (r6) the library issues the exchange itself (sim_exchange_init): the slab this shard addresses to itself goes straight to where the
  // round's exchange would have put it — slab `rank` of chunk c's region of the receive buffer of tick t — and sim_exchange_chunk leaves it out
  uint4* self_slab = h->self_direct ? h->rbuf[t & 1] + ((size_t)c * x.V + d.shard_rank) * x.slab_u * 4u : nullptr;
  rfx_meta_kernel<<<grid_for(((size_t)((x.M & 15u) ? x.M : x.M >> 4) + (size_t)x.NBh + 16u) * x.V), BLOCK, 0, h->stream>>>(x, h->rf_cntb[t % 3] + (size_t)c * d.N, h->rf_btot[t % 3] + (size_t)c * x.V * x.NBh, xoff, (u32)t, send, d.shard_rank, self_slab);
  // (r6) the tick's LAST pack carries the event that marks "tick t has finished" (what sim_step_end would record behind it: the build
  // stream waits for it before it overwrites what this pack read) as the stop event of its dispatch — a marker packet less per tick
  hipEvent_t e1 = (d.swim && h->in_tick && t == h->tick && c + 1u == x.C) ? h->sreq_ev[t % 3] : nullptr;
  launch_ev(rfx_pack_kernel, grid_for((size_t)per * 4u), BLOCK, h->stream, nullptr, e1, x, h->rf_rsrc[t % 3] + (size_t)c * per, xoff, d.obox[0], d.Nl, send, d.shard_rank, self_slab);
  if (e1) {
    h->sreq_wait[t % 3] = e1;
    h->sreq_on_dispatch = true;
  }
  HCHECK(hipGetLastError());
  return SIM_OK;
}
// ---- sim_step_begin, step by step (in this order; a step that fails returns its code) ----
// 1. every shard is here: the slot-less suspicions / reconnect attempts of the tick BEFORE the one that just ended are replayed now —
// behind whatever the caller scheduled for this tick so far, which is where a sharded host (sim_suspect_import at the start of its
// step) puts them too
static int begin_replay(sim_handle* h) {
  static thread_local std::vector<u32> buf(2 * SIM_SUSPECT_REQ_MAX);
  u32 n = 0;
  int rc = sim_suspect_requests(h, buf.data(), SIM_SUSPECT_REQ_MAX, &n);
  if (rc) return rc;
  for (u32 i = 0; i < n; ++i)
    if ((rc = inject_val(h, h->tick, SIM_OP_SUSPECT, buf[2 * i], buf[2 * i + 1], 0, 0)) != SIM_OK) return rc;
  return SIM_OK;
}
// 2. the recycling pass, when one is due
static int begin_recycle(sim_handle* h) {
  if (!recycle_is_due(h)) return SIM_OK;
  if (h->d.sharded) return SIM_ESTATE;  // the host runs the pass first (it needs every shard's verdict)
  return recycle_local(h);
}
// 3. this tick's request list: its count was zeroed by the previous tick's kernel (or never used); the two other buffers hold the
// lists of the two ticks before until they have been read
static void begin_requests(sim_handle* h) {
  Dev& d = h->d;
  d.sreq = h->sreq_buf[h->tick % 3];
  d.sreq_next = h->sreq_buf[(h->tick + 1) % 3];
  d.sreq_hh = d.sharded ? nullptr : h->sreq_host[h->tick % 3];
}
// 4. cur_tp := the parameters of tick h->tick (n_slots: behind the operations)
static void begin_params(sim_handle* h) {
  TickP& tp = h->cur_tp;
  tickp_make(&tp, &h->cfg, h->tick);
#ifdef TICK_ABLATE
  tp.abl = g_ablate;
#endif
  for (u32 k = 0; k < SIM_MAX_FANOUT; ++k) { tp.prot[k] = h->prev.rot[k]; tp.prho[k] = h->prev.rho[k]; }
  if (h->d.sharded) h->d.xrecv = h->rbuf[(h->tick + 1) & 1];  // what was sent during tick - 1
}
// 5a. the query's filter entry: started by the first filter operation that names the query, SEALED by its SIM_OP_QUERY (word 3),
// replaced by whatever names another query with the same residue — or the same id again once the entry is sealed: a query issued a
// second time under an id starts from no filters.  The host's copy, and the device's when it changed; false: the id does not fit
static bool op_query_filter(sim_handle* h, const OpEnt& e) {
  u32* f = h->qfilt.data() + (size_t)(e.a % SIM_QT) * SIM_QF_WORDS;
  bool changed = false;
  if (f[0] != e.a || (f[3] & 1u)) { memset(f, 0, SIM_QF_WORDS * 4); f[0] = e.a; f[2] = 0xFFFFFFFFu; changed = true; }
  if (e.op == SIM_OP_QUERY_FILTER_ID) {
    if (f[1] == SIM_QF_IDS) return false;
    f[4 + f[1]++] = e.b; changed = true;
  } else if (e.op == SIM_OP_QUERY_FILTER_TAGS) { f[2] &= e.b; changed = true; }
  else { f[3] |= 1u; changed = true; }
  if (changed) {
    QFiltEnt qe;
    memcpy(&qe, f, sizeof qe);
    qfilt_set_kernel<<<1, 64, 0, h->stream>>>(QFILT(h->d) + (size_t)(e.a % SIM_QT) * (SIM_QF_WORDS / 4), qe);
  }
  return true;
}
// 5. the operations scheduled up to this tick, in ops_kernel batches of 8; rc_req := its reconnect attempts (node, target), in schedule order
static int begin_ops(sim_handle* h, std::vector<u32>& rc_req) {
  Dev& d = h->d;
  TickP& tp = h->cur_tp;
  while (h->op_cursor < h->ops.size() && h->ops[h->op_cursor].tick <= h->tick) {
    OpBatch ob;
    memset(&ob, 0, sizeof ob);
    while (ob.n < 8 && h->op_cursor < h->ops.size() && h->ops[h->op_cursor].tick <= h->tick) {
      const OpEnt& e = h->ops[h->op_cursor++];
      if (e.op == SIM_OP_RECONNECT) { rc_req.push_back(e.node); rc_req.push_back(e.a); continue; }  // resolved once the tick's operations have run
      if (e.op == SIM_OP_QUERY_FILTER_ID || e.op == SIM_OP_QUERY_FILTER_TAGS || e.op == SIM_OP_QUERY) {
        if (!op_query_filter(h, e)) { h->ops_dropped++; continue; }  // model bound
        if (e.op != SIM_OP_QUERY) continue;
      }
      u32 x = op_subject(h, e.op, e.node, e.a, e.b);
      if (x != NOSLOT) {
        const int src = ensure_slot(h, x);
        if (src == SIM_ENOSLOT) { h->ops_dropped++; continue; }  // no free view slot: the operation does not happen (model bound, counted)
        if (src != SIM_OK) return src;  // out of memory / a device error while a plane was being mapped is NOT a model drop (ADVICE r5)
      }
      if (e.op == SIM_OP_JOIN && (h->cfg.flags & SIM_CF_JOIN_SYNC) && e.node >= d.shard0 && e.node < d.shard0 + d.Nl) {
        // memberlist.join comes first: what was batched so far runs, then the joining node adopts its partner's view
        if (ob.n) ops_kernel<<<1, 64, 0, h->stream>>>(d, ob, h->tick, d.N > 1 ? 1u : 0u, tp.query_base, h->q_timeout);
        memset(&ob, 0, sizeof ob);
        join_sync_kernel<<<1, BLOCK, 0, h->stream>>>(d, (u32)h->walk.size(), e.node, e.a, (u32)h->tick);
      }
      ob.op[ob.n] = e.op; ob.node[ob.n] = e.node; ob.a[ob.n] = e.a; ob.b[ob.n] = e.b; ob.val[ob.n] = e.val;
      if (e.op == SIM_OP_QUERY) {  // a fresh tracker: who acked / responded starts empty
        u32 j = e.a % SIM_QT;
        size_t words = ((size_t)d.N + 31) / 32;
        ob.c[ob.n] = j;
        HCHECK(hipMemsetAsync(d.qbits + (size_t)j * 2 * words, 0, 2 * words * 4, h->stream));
      }
      ob.n++;
    }
    if (ob.n) ops_kernel<<<1, 64, 0, h->stream>>>(d, ob, h->tick, d.N > 1 ? 1u : 0u, tp.query_base, h->q_timeout);
  }
  tp.n_slots = (u32)h->walk.size();  // after the operations: they may have taken slots
  return SIM_OK;
}
// 6. The tick's SIM_OP_RECONNECT operations -> the push-pull pairs that run in this tick, rc_a / rc_b (oracle rc_resolve): an attempt
// whose initiator or target is not running fails and is forgotten; the pairs of a tick are disjoint and do not share the tick with a
// push-pull batch — an attempt that would goes back on the schedule for the next tick.
static int begin_reconnects(sim_handle* h, const std::vector<u32>& rc_req) {
  Dev& d = h->d;
  h->rc_a.clear(); h->rc_b.clear();
  if (rc_req.empty()) return SIM_OK;
  std::vector<u32> up(((size_t)d.N + 31) / 32);  // ground-truth liveness after this tick's operations (rare path: a copy and a wait)
  HCHECK(hipMemcpyAsync(up.data(), d.upmap, up.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  auto is_up = [&](u32 g) { return (up[g >> 5] >> (g & 31)) & 1u; };
  u32 cls;
  const bool batch = pp_batch_class(h, &cls);
  for (size_t i = 0; i + 1 < rc_req.size(); i += 2) {
    const u32 a = rc_req[i], b = rc_req[i + 1];
    if (a == b || !is_up(a) || !is_up(b)) continue;
    bool busy = batch;
    for (size_t j = 0; j < h->rc_a.size() && !busy; ++j) busy = h->rc_a[j] == a || h->rc_b[j] == a || h->rc_a[j] == b || h->rc_b[j] == b;
    if (busy) { int rc = inject_val(h, h->tick + 1, SIM_OP_RECONNECT, a, b, 0, 0); if (rc) return rc; }
    else { h->rc_a.push_back(a); h->rc_b.push_back(b); }
  }
  return SIM_OK;
}
// 7. every shard is here: the tick's push-pull batch, then the Reconnector's push-pulls (none on a batch tick); sharded: the host runs both, sim_pp_*
static void begin_pushpull(sim_handle* h) {
  Dev& d = h->d;
  const TickP& tp = h->cur_tp;
  if (h->pp_step && h->tick > 0 && h->tick % h->pp_step == 0) {
    u32 cls = (u32)((h->tick / h->pp_step) % PP_GROUPS);
    u32 half = tp.N / 2, n_pairs = half > cls ? (half - cls + PP_GROUPS - 1) / PP_GROUPS : 0;
    if (n_pairs) pushpull_kernel<<<(n_pairs + 63) / 64, 64, 0, h->stream>>>(d, tp, cls, n_pairs, split_mapped(h->sp[SP_EV]) - d.X);
  }
  for (size_t i = 0; i < h->rc_a.size(); i += 8) {
    PairBatch pb;
    memset(&pb, 0, sizeof pb);
    for (size_t j = i; j < h->rc_a.size() && j < i + 8; ++j) { pb.a[pb.n] = h->rc_a[j]; pb.b[pb.n++] = h->rc_b[j]; }
    pp_pairs_kernel<<<1, 64, 0, h->stream>>>(d, tp, pb, split_mapped(h->sp[SP_EV]) - d.X);
  }
}
// 9. kRandomNodes: the graph of the packets this tick RECEIVES — sent during tick - 1 — stands; the graphs ahead are enqueued; rf_skip
static int begin_graph(sim_handle* h) {
  Dev& d = h->d;
  if (d.sharded) {
    // a shard: the rows of this tick come from the slabs the round's exchange delivered (sim_exchange_wait / the host's
    // collective has completed): one launch (rfx_index_kernel); an entry = a cell of the receive buffer
    const uint4* rb = h->rbuf[(h->tick + 1) & 1];
    if (h->tick > 0) rfx_index_kernel<<<h->rfx.NBh, RFX_T, rfx_index_lds(h->rfx), h->stream>>>(h->rfx, rb, d.Nl, h->rx_cap, h->rx_rcsr, h->rx_rsrc, h->xflag);
    d.rcsr = h->rx_rcsr;  // (tick 0: zeros — nothing has been sent)
    d.rsrc = h->rx_rsrc;
    d.rfrd = rb;
    d.NC = 1u;            // the pages of a packet are adjacent cells of its slab
  } else {
    if (int rc = h->tick > 0 ? rf_ready(h, h->tick - 1) : SIM_OK) return rc;
    d.rcsr = h->rf_rcsr[(h->tick + 2) % 3];  // (tick 0: a buffer of zeros — nothing has been sent)
    d.rsrc = h->rf_rsrc[(h->tick + 2) % 3];
    d.rfrd = d.obox[h->tick & 1];  // ... and the cells those packets sit in: this handle's own of the tick before
    d.NC = d.Nl;
  }
  if (int rc = h->rf_sync ? SIM_OK : rf_look_ahead(h)) return rc;
  if (d.gttd) {
    RfP r = h->rfp;
    r.rb = rng_base(h->cfg.seed, STREAM_RFAN, h->tick); r.feff = h->cur_tp.feff;
    rf_skip_kernel<<<grid_for(d.Nl), BLOCK, 0, h->stream>>>(d, h->cur_tp, r, h->d_base);
  }
  return SIM_OK;
}
// 10. Timing of the tick's launch(es) with HIP events.  One launch per tick: the pair rides on the dispatch itself
// (hipExtLaunchKernelGGL: start / stop = the kernel's own begin and end, no barrier packets in the stream — two
// hipEventRecord calls around every launch cost 10 us of stream time each tick).  Several chunk launches per tick
// (sharded, C > 1): the pair brackets them with hipEventRecord.
static int begin_timing(sim_handle* h) {
  h->tick_timed = h->profiling && (h->prof_seq++ % h->profiling) == 0;
  h->tick_bracket = h->tick_timed && h->d.sharded && h->cur_tp.C > 1;
  if (h->tick_bracket) {
    HCHECK(hipEventCreate(&h->tick_ev0));
    HCHECK(hipEventRecord(h->tick_ev0, h->stream));
  }
  return SIM_OK;
}
// ---- the tick's launches ----
static int tick_launch(sim_handle* h, u32 chunk) {
  Dev& d = h->d;
  const TickP& tp = h->cur_tp;
  const TickP& ptp = h->tick ? h->prev : h->cur_tp;  // the map the packets in flight were sent with (tick 0: none are)
  u32 cnt = chunk == 0xFFFFFFFFu ? d.Nl : tp.V * tp.sub;
  int grid = (int)((cnt + TBLOCK - 1) / TBLOCK);
  u32 cur = (u32)(h->tick & 1);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h->tick_timed && !h->tick_bracket) {
    HCHECK(hipEventCreate(&e0));
    HCHECK(hipEventCreate(&e1));
    h->prof.emplace_back(e0, e1);
  }
  // One launch per tick and a request list to read behind it (local mode, SWIM on): the event the host waits on before it
  // reads the list rides on the dispatch as its stop event — a hipEventRecord behind every launch is a marker packet of
  // its own, ~5 us of stream time per tick.
  h->sreq_on_dispatch = false;
  if (d.swim && !d.sharded && chunk == 0xFFFFFFFFu) {
    if (!e1) e1 = h->sreq_ev[h->tick % 3];
    h->sreq_wait[h->tick % 3] = e1;
    h->sreq_on_dispatch = true;
  }
  auto go = [&](auto kernel) { launch_ev(kernel, grid, TBLOCK, h->stream, e0, e1, d, tp, ptp, cur, h->d_base, chunk, cnt); };
  // (the kernels are emitted in the order these lines first name them: the four local fan-outs, then the four sharded ones)
#define TICK_LOCAL(FF)                                                                                                   \
  do {                                                                                                                   \
    if (d.rfan) { if (d.PG > 1u) go(tick_kernel<false, FF, false, true, true>); else go(tick_kernel_rf<FF>); }           \
    else if (tp.B == 64u) { if (d.PG > 1u) go(tick_kernel<false, FF, true, true>); else go(tick_kernel<false, FF, true, false>); } \
    else { if (d.PG > 1u) go(tick_kernel<false, FF, false, true>); else go(tick_kernel<false, FF, false, false>); }      \
  } while (0)
#define TICK_SHARD(FF) do { if (d.PG > 1u) go(tick_kernel<true, FF, false, true>); else go(tick_kernel<true, FF, false, false>); } while (0)
  switch (tp.feff + ((d.sharded && !d.rfan) ? 4u : 0u)) {  // one instantiation per fan-out: the drain loop is fully unrolled
    // (the random fan-out on a shard runs the local instantiation: its packets stay in its cells, the exchange gathers them)
    case 0: case 1: TICK_LOCAL(1); break;
    case 2: TICK_LOCAL(2); break;
    case 3: TICK_LOCAL(3); break;
    case 4: TICK_LOCAL(4); break;
    case 5: TICK_SHARD(1); break;
    case 6: TICK_SHARD(2); break;
    case 7: TICK_SHARD(3); break;
    default: TICK_SHARD(4); break;
  }
#undef TICK_SHARD
#undef TICK_LOCAL
  // the nodes this launch left to the second level of the queue (deep, or about to be): their phase 2, on the launch's list.  The
  // grid follows the longest list seen so far (a pinned word the kernel keeps: read without waiting, a tick or two late — any grid
  // is correct, the list is walked in strides); with nobody ever on a list it is 64 waves that read one word each and leave.
  const u32 seen = *(volatile u32*)h->deep_seen;
  const u32 want = std::max<u32>(64u, 2u * ((seen + TBLOCK - 1) / TBLOCK));
  const u32 dgrid = std::min<u32>(want, (d.Nl + TBLOCK - 1) / TBLOCK);
  deep_queue_kernel<<<std::max<u32>(dgrid, 1u), TBLOCK, 0, h->stream>>>(d, tp, cur, h->deep_seen);
  d.deep_par ^= 1u;
  HCHECK(hipGetLastError());
  return SIM_OK;
}
// launch sender chunk `chunk` (0xFFFFFFFF: every node at once); random fan-out on a shard: pack the slabs of the round's exchange from the cells it fills
static int chunk_run(sim_handle* h, u32 chunk) {
  int rc = tick_launch(h, chunk);
  if (rc == SIM_OK && h->d.sharded && h->d.rfan) rc = rfx_pack(h, h->tick, chunk == 0xFFFFFFFFu ? 0u : chunk);
  return rc;
}
// the list of one finished tick out of its buffer (sorted by prober); marks it read
static int sreq_take(sim_handle* h, u64 t, uint32_t* out, uint32_t cap_pairs, uint32_t* n_pairs) {
  *n_pairs = 0;
  const u32 b = (u32)(t % 3);
  if (h->sreq_tick[b] != t) return SIM_OK;  // nothing recorded for that tick, or read already
  h->sreq_tick[b] = ~0ull;
  if (hipEvent_t done = tick_done_event(h, t)) HCHECK(hipEventSynchronize(done));
  u32* hh = h->sreq_host[b];
  u32 n = 0;
  if (!h->d.sharded) {  // the kernel wrote the head of the list here itself
    while (n < SREQ_HEAD && hh[2 * n] != 0xFFFFFFFFu) ++n;
    if (!n) return SIM_OK;
  }
  if (h->d.sharded || n == SREQ_HEAD) {  // a long list (or no host copy): the buffer on the device is untouched until the tick after next has run
    HCHECK(hipMemcpyAsync(&n, h->sreq_buf[b], 4, hipMemcpyDeviceToHost, h->stream));
    HCHECK(hipStreamSynchronize(h->stream));
  }
  auto forget = [&]() { if (!h->d.sharded) memset(hh, 0xFF, 2 * SREQ_HEAD * 4); };
  if (!n) return SIM_OK;
  if (n > SIM_SUSPECT_REQ_MAX) { h->ops_dropped += n; forget(); return SIM_OK; }  // model bound: the whole tick's list is dropped
  if (n > cap_pairs || !out) { h->sreq_tick[b] = t; return SIM_ERANGE; }
  if (!h->d.sharded && n <= SREQ_HEAD) memcpy(out, hh, (size_t)n * 8);
  else {
    HCHECK(hipMemcpyAsync(out, h->sreq_buf[b] + 1, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    HCHECK(hipStreamSynchronize(h->stream));
  }
  forget();
  std::vector<std::pair<u32, u32>> v(n);
  for (u32 i = 0; i < n; ++i) v[i] = {out[2 * i], out[2 * i + 1]};
  std::sort(v.begin(), v.end());  // a node probes once per tick: probers are distinct
  for (u32 i = 0; i < n; ++i) { out[2 * i] = v[i].first; out[2 * i + 1] = v[i].second; }
  *n_pairs = n;
  return SIM_OK;
}

extern "C" {
// One tick = sim_step_begin (operations, push-pull batch, tick parameters), one tick-kernel launch per sender chunk
// (sim_step_chunk; a single launch when there is one chunk or all shards are local), sim_step_end.  sim_step does all
// of it; a sharded host that wants the exchange of chunk c in flight while chunk c + 1 computes drives the three
// calls itself (serf_amd/shard.py).
int sim_step_begin(sim_handle* h) {
  if (!h) return SIM_EINVAL;
  Dev& d = h->d;
  if (h->in_tick || (d.sharded && !h->bound)) return SIM_ESTATE;
  if (h->tick > SIM_TICK_MAX) return SIM_ERANGE;  // the last tick a handle executes (include/serf_sim.h)
  if (h->xflag && *h->xflag) return SIM_ERANGE;  // a slab of the random fan-out's exchange (or a count byte, or the rows) overflowed
  if (h->xpending) { int rc = sim_exchange_wait(h); if (rc) return rc; }  // the packets of the round before have landed
  if (int rc = (d.swim && !d.sharded) ? begin_replay(h) : SIM_OK) return rc;
  if (int rc = begin_recycle(h)) return rc;
  if (d.swim) begin_requests(h);
  begin_params(h);
  std::vector<u32> rc_req;
  if (int rc = begin_ops(h, rc_req)) return rc;
  if (int rc = begin_reconnects(h, rc_req)) return rc;
  if (!d.sharded) begin_pushpull(h);
  if (d.gttd && !d.rfan) gossip_skip_kernel<<<grid_for(d.Nl), BLOCK, 0, h->stream>>>(d, h->cur_tp, h->d_base);  // 8. whom not to gossip to this tick
  if (int rc = d.rfan ? begin_graph(h) : SIM_OK) return rc;
  if (int rc = begin_timing(h)) return rc;
  h->in_tick = true;
  return SIM_OK;
}
int sim_step_chunk(sim_handle* h, uint32_t chunk) {
  if (!h) return SIM_EINVAL;
  if (!h->in_tick) return SIM_ESTATE;
  if (!h->d.sharded || chunk >= h->cur_tp.C) return SIM_EINVAL;
  if (sim_pp_due(h) > 0) return SIM_ESTATE;  // the push-pull batch of this tick comes first (its pairs span shards: the host runs it)
  return chunk_run(h, h->cur_tp.C == 1 ? 0xFFFFFFFFu : chunk);
}
int sim_step_end(sim_handle* h) {
  if (!h) return SIM_EINVAL;
  if (!h->in_tick) return SIM_ESTATE;
  if (h->tick_bracket) {
    hipEvent_t ev1 = nullptr;
    HCHECK(hipEventCreate(&ev1));
    HCHECK(hipEventRecord(ev1, h->stream));
    h->prof.emplace_back(h->tick_ev0, ev1);
  }
  h->prev = h->cur_tp;
  h->tick++;
  h->in_tick = false;
  // Slot-less failed probes: the head of this tick's list follows the launch into pinned memory; the list of the tick
  // BEFORE is read now (its copy landed a whole tick ago) and, every shard being here, replayed next tick.
  if (h->d.swim) {
    const u64 t = h->tick - 1;  // the tick that just ended
    if (!h->sreq_on_dispatch) {
      HCHECK(hipEventRecord(h->sreq_ev[t % 3], h->stream));
      h->sreq_wait[t % 3] = h->sreq_ev[t % 3];
    }
    h->sreq_on_dispatch = false;
    h->sreq_tick[t % 3] = t;
  }
  if (h->trk) { if (int rc = track_step_end(h)) return rc; }  // registered trackers: the tick's evaluation follows it on the stream
  return observers_step_end(h);  // running series, census, roll, ledger: the tick's sample, when one is due, likewise
}
int sim_suspect_export(sim_handle* h, void* out) {  // the head of the list of the tick that just ended -> device memory of the caller
  if (!h || !out || h->in_tick || !h->tick) return SIM_EINVAL;
  static_assert(SIM_SREQ_HEAD_WORDS * 4 <= (1 + 2 * SIM_SUSPECT_REQ_MAX) * 4, "the head is a prefix of the list buffer");
  if (!h->d.swim) { HCHECK(hipMemsetAsync(out, 0, SIM_SREQ_HEAD_WORDS * 4, h->stream)); return SIM_OK; }
  const u64 t = h->tick - 1;
  HCHECK(hipMemcpyAsync(out, h->sreq_buf[t % 3], SIM_SREQ_HEAD_WORDS * 4, hipMemcpyDeviceToDevice, h->stream));
  h->sreq_tick[t % 3] = ~0ull;  // handed over: nothing for sim_suspect_requests to read
  return SIM_OK;
}
int sim_suspect_import(sim_handle* h, uint64_t of_tick, const uint32_t* heads, uint32_t world) {
  if (!h || !world || h->in_tick || of_tick + 2 < h->tick) return SIM_EINVAL;
  if (!heads) {  // (r6) the heads the library's own exchange carried (sim_exchange_chunk): pinned host memory, marked by an event
    if (!h->xh_host || world != h->xworld) return SIM_EINVAL;
    const u32 i = (u32)(of_tick % 4);
    if (h->xh_tick[i] != of_tick) return SIM_ESTATE;  // no exchange of that tick was issued (or its heads were imported already)
    HCHECK(hipEventSynchronize(h->xh_ev[i]));
    h->xh_tick[i] = ~0ull;
    heads = h->xh_host + (size_t)i * world * SIM_SREQ_HEAD_WORDS;
  }
  std::vector<std::pair<u32, u32>> v;
  u64 total = 0;
  for (u32 w = 0; w < world; ++w) total += heads[(size_t)w * SIM_SREQ_HEAD_WORDS];
  if (total > SIM_SUSPECT_REQ_MAX) { h->ops_dropped += (u32)total; return SIM_OK; }  // model bound, the single-process handle's: the whole tick's list is dropped
  for (u32 w = 0; w < world; ++w) {
    const u32* hd = heads + (size_t)w * SIM_SREQ_HEAD_WORDS;
    for (u32 i = 0; i < hd[0]; ++i) v.emplace_back(hd[1 + 2 * i], hd[2 + 2 * i]);
  }
  std::sort(v.begin(), v.end());
  for (auto& pr : v) {
    int rc = inject_val(h, of_tick + 2, SIM_OP_SUSPECT, pr.first, pr.second, 0, 0);
    if (rc) return rc;
  }
  return SIM_OK;
}
int sim_suspect_requests(sim_handle* h, uint32_t* out, uint32_t cap_pairs, uint32_t* n_pairs) {
  if (!h || !n_pairs || h->in_tick) return SIM_EINVAL;
  *n_pairs = 0;
  if (!h->d.swim || h->tick < 2) return SIM_OK;
  return sreq_take(h, h->tick - 2, out, cap_pairs, n_pairs);  // the requests of the tick BEFORE the one that just ended
}
int sim_step(sim_handle* h, uint32_t n_ticks) {
  if (!h) return SIM_EINVAL;
  if (n_ticks && h->tick + n_ticks - 1 > SIM_TICK_MAX) return SIM_ERANGE;  // the whole of n_ticks first: nothing is executed
  Dev& d = h->d;
  if (d.sharded && !h->bound) return SIM_ESTATE;
  if (d.sharded && n_ticks > 1) return SIM_EINVAL;  // the caller has to move send -> recv between two ticks
  for (u32 it = 0; it < n_ticks; ++it) {
    if (sim_pp_due(h) > 0) return SIM_ESTATE;  // needs the host between begin and end (cross-shard push-pull batch)
    int rc = sim_step_begin(h);
    if (rc) return rc;
    if (d.sharded && h->cur_tp.C > 1)
      for (u32 c = 0; c < h->cur_tp.C && rc == SIM_OK; ++c) rc = chunk_run(h, c);
    else rc = chunk_run(h, 0xFFFFFFFFu);
    int rc2 = sim_step_end(h);
    if (rc) return rc;
    if (rc2) return rc2;
  }
  return SIM_OK;
}
int sim_sync(sim_handle* h) {
  if (!h) return SIM_EINVAL;
  if (h->xcomm && h->xpending) { int rc = sim_exchange_wait(h); if (rc) return rc; }  // (the exchange stream's work is the handle's as well)
  HCHECK(hipStreamSynchronize(h->stream));
  // the packed exchange's overflow flag (pinned, written by the rf / rfx kernels): sim_step_begin sees it a tick late and without
  // waiting — here the stream is idle, so an overflow of the LAST tick is reported as well (ADVICE r5)
  if (h->xflag && *h->xflag) return SIM_ERANGE;
  return SIM_OK;
}
}  // extern "C"
