// serf_sim_exchange.inc — part of the translation unit serf_sim.hip (included from there, in this order; not a header of its own).
// host: the exchange buffers of a shard and the round's all-to-all over RCCL (inside extern "C").
// bytes of the handle's send buffer (and of each receive buffer): the slabs [C][V dst][fp][M / V / C] of 48-byte packets — or,
// random fan-out on a shard, the V packed slabs (RfxL: header, count bytes, bucket totals, 64-byte cells)
static size_t xsend_bytes(const sim_handle* h) {
  const Dev& d = h->d;
  if (!d.sharded) return 0;
  return d.rfan ? (size_t)h->rfx.C * d.V * h->rfx.slab_u * 64u : (size_t)d.fp * d.M * sizeof(sim_packet);
}
int sim_exchange_bytes(const sim_handle* h, size_t* bytes) {
  if (!h || !bytes) return SIM_EINVAL;
  *bytes = xsend_bytes(h);
  return SIM_OK;
}
int sim_exchange_layout(const sim_handle* h, uint32_t* kind, uint32_t* planes, size_t* send_plane_bytes, size_t* recv_bytes) {
  if (!h || !kind || !planes || !send_plane_bytes || !recv_bytes) return SIM_EINVAL;
  const Dev& d = h->d;
  *kind = (d.sharded && d.rfan) ? SIM_XCHG_PACKED : SIM_XCHG_ALL_TO_ALL;
  *planes = 1;
  *send_plane_bytes = *recv_bytes = xsend_bytes(h);
  return SIM_OK;
}
int sim_bind_exchange2(sim_handle* h, void* send, void* recv0, void* recv1) {
  if (!h || !h->d.sharded || !send || !recv0 || !recv1) return SIM_EINVAL;
  h->d.xsend = (uint4*)send;
  h->rbuf[0] = (uint4*)recv0;
  h->rbuf[1] = (uint4*)recv1;
  h->d.xrecv = h->rbuf[(h->tick + 1) & 1];
  // (all zero: no packets — the bijection's empty cells, the random fan-out's empty slabs)
  HCHECK(hipMemsetAsync(send, 0, xsend_bytes(h), h->stream));
  HCHECK(hipMemsetAsync(recv0, 0, xsend_bytes(h), h->stream));
  if (recv1 != recv0) HCHECK(hipMemsetAsync(recv1, 0, xsend_bytes(h), h->stream));
  h->bound = true;
  return SIM_OK;
}
int sim_bind_exchange(sim_handle* h, void* send, void* recv) { return sim_bind_exchange2(h, send, recv, recv); }
int sim_bind_exchange3(sim_handle* h, void* send, size_t send_bytes, void* recv0, void* recv1, size_t recv_bytes) {
  if (!h || !h->d.sharded || send_bytes < xsend_bytes(h) || recv_bytes < xsend_bytes(h)) return SIM_EINVAL;
  return sim_bind_exchange2(h, send, recv0, recv1);
}
int sim_exchange_chunks(const sim_handle* h, uint32_t* chunks, size_t* bytes_per_chunk) {
  if (!h || !chunks || !bytes_per_chunk) return SIM_EINVAL;
  u32 C = h->cfg.chunks ? h->cfg.chunks : 1;
  *chunks = h->d.sharded ? C : 1;
  *bytes_per_chunk = xsend_bytes(h) / C;
  return SIM_OK;
}

// ---- the round's all-to-all over RCCL, issued by the library (include/serf_sim.h sim_exchange_*; SURVEY.md §8e) ----
#define NCHECK(x)                                                                                          \
  do {                                                                                                     \
    ncclResult_t r_ = (x);                                                                                 \
    if (r_ != ncclSuccess) {                                                                               \
      fprintf(stderr, "serf_sim: %s failed: %s (%s:%d)\n", #x, ncclGetErrorString(r_), __FILE__, __LINE__); \
      return SIM_EDEVICE;                                                                                  \
    }                                                                                                      \
  } while (0)
static_assert(sizeof(ncclUniqueId) <= SIM_EXCHANGE_ID_BYTES, "the communicator id travels as SIM_EXCHANGE_ID_BYTES bytes");
int sim_exchange_unique_id(uint8_t* id_out) {
  if (!id_out) return SIM_EINVAL;
  ncclUniqueId id;
  NCHECK(ncclGetUniqueId(&id));
  memset(id_out, 0, SIM_EXCHANGE_ID_BYTES);
  memcpy(id_out, &id, sizeof id);
  return SIM_OK;
}
int sim_exchange_library(char* buf, size_t cap) {
  if (!buf || cap < 16) return SIM_EINVAL;
  int v = 0;
  NCHECK(ncclGetVersion(&v));  // major * 10000 + minor * 100 + patch
  snprintf(buf, cap, "RCCL %d.%d.%d", v / 10000, (v / 100) % 100, v % 100);
  return SIM_OK;
}
int sim_exchange_init(sim_handle* h, const uint8_t* id, uint32_t rank, uint32_t world) {
  if (!h || !id) return SIM_EINVAL;
  Dev& d = h->d;
  if (!d.sharded || world != h->cfg.shard_count || rank != h->cfg.shard_rank) return SIM_EINVAL;
  if (!h->bound || h->xcomm) return SIM_ESTATE;
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof uid);
  HCHECK(hipSetDevice(h->device));
  NCHECK(ncclCommInitRank(&h->xcomm, (int)world, uid, (int)rank));
  HCHECK(hipStreamCreateWithFlags(&h->xstream, hipStreamNonBlocking));
  HCHECK(hipEventCreateWithFlags(&h->xev_go, hipEventDisableTiming));
  HCHECK(hipEventCreateWithFlags(&h->xev_done, hipEventDisableTiming));
  h->xworld = world;
  const char* xhe = getenv("SERF_SIM_XHEADS");  // (= 0: the host hands the lists over itself — sim_suspect_export / a collective of its own / sim_suspect_import)
  if (d.swim && !(xhe && *xhe == '0')) {  // (r6) the suspicion lists' heads travel with the round's exchange: see sim_handle::xh_dev
    const size_t bytes = (size_t)4u * world * SIM_SREQ_HEAD_WORDS * 4u;
    HCHECK(hipMalloc((void**)&h->xh_dev, bytes));
    h->allocs.push_back(h->xh_dev);
    HCHECK(hipMemsetAsync(h->xh_dev, 0, bytes, h->stream));
    HCHECK(hipHostMalloc((void**)&h->xh_host, bytes, hipHostMallocDefault));
    memset(h->xh_host, 0, bytes);
    for (int i = 0; i < 4; ++i) { HCHECK(hipEventCreateWithFlags(&h->xh_ev[i], hipEventDisableTiming)); h->xh_tick[i] = ~0ull; }
  }
  h->self_direct = d.rfan != 0u;  // (the packed slabs: rfx_pack writes slab `rank` straight into the receive buffer, sim_exchange_chunk leaves it out)
  return SIM_OK;
}
int sim_exchange_chunk(sim_handle* h, uint32_t chunk) {
  if (!h) return SIM_EINVAL;
  if (!h->xcomm) return SIM_ESTATE;
  Dev& d = h->d;
  const u32 C = h->cfg.chunks ? h->cfg.chunks : 1, V = h->xworld;
  if (chunk >= C) return SIM_EINVAL;
  // (called behind sim_step_chunk(chunk), before or after sim_step_end: the packets sent during tick t land in recv[t & 1])
  const u64 t = h->in_tick ? h->tick : h->tick - 1;
  const size_t chunk_bytes = xsend_bytes(h) / C, slab = chunk_bytes / V;  // (random fan-out: the V packed slabs, one chunk)
  const uint8_t* send = reinterpret_cast<const uint8_t*>(d.xsend) + (size_t)chunk * chunk_bytes;
  uint8_t* recv = reinterpret_cast<uint8_t*>(h->rbuf[t & 1]) + (size_t)chunk * chunk_bytes;
  // One chunk per tick: there is no later launch for the exchange to travel beside — it goes on the handle's own stream, between the
  // pack and the next tick's index pass, and nothing hops between streams (r6: a hop = an event recorded on one stream and waited for
  // on another costs 30 - 50 us of latency here, two of them per tick: profiles/r06_experiments.md §7).
  // Several chunks: the exchange stream waits for what the handle's stream holds now — this chunk's launch —, not for the chunks after it.
  const bool inl = C == 1;
  hipStream_t xs = inl ? h->stream : h->xstream;
  if (!inl) {
    HCHECK(hipEventRecord(h->xev_go, h->stream));
    HCHECK(hipStreamWaitEvent(h->xstream, h->xev_go, 0));
  }
  // (r6) behind the tick's LAST launch the list of its slot-less suspicions is complete: its head goes to every peer in the same group
  // (32 KiB a peer), and what the heads hold follows into pinned host memory — sim_suspect_import(h, t, NULL, world) reads it at tick t + 2
  const bool heads = h->xh_dev && chunk + 1u == C;
  const u32* myhead = h->sreq_buf[t % 3];
  u32* hdev = heads ? h->xh_dev + (size_t)(t % 4) * V * SIM_SREQ_HEAD_WORDS : nullptr;
  NCHECK(ncclGroupStart());
  for (u32 p = 0; p < V; ++p) {
    if (heads && p != d.shard_rank) {
      NCHECK(ncclSend(myhead, SIM_SREQ_HEAD_WORDS, ncclUint32, (int)p, h->xcomm, xs));
      NCHECK(ncclRecv(hdev + (size_t)p * SIM_SREQ_HEAD_WORDS, SIM_SREQ_HEAD_WORDS, ncclUint32, (int)p, h->xcomm, xs));
    }
    if (h->self_direct && p == d.shard_rank) continue;  // (packed slabs: the pack wrote this shard's own slab straight into the receive buffer — rfx_pack)
    NCHECK(ncclSend(send + (size_t)p * slab, slab, ncclUint8, (int)p, h->xcomm, xs));
    NCHECK(ncclRecv(recv + (size_t)p * slab, slab, ncclUint8, (int)p, h->xcomm, xs));
  }
  NCHECK(ncclGroupEnd());
  if (heads) {
    // (the event rides on the dispatch as its stop event: no marker packet of its own between the pack and the next tick's index pass)
    // One chunk, random fan-out: the copy to the host runs on the BUILD stream (a hardware queue of its own), behind the event the pack's
    // dispatch carries (V == 1: nothing else wrote what it reads) or a marker behind the group — the handle's stream holds neither the
    // kernel nor the two gaps around it (14 + 4 + 10 us of every tick on one rank); the host reads the result two ticks later.
    hipStream_t hs = xs;
    if (inl && h->rf_stream) {
      hipEvent_t ev = V == 1u ? tick_done_event(h, t) : nullptr;
      if (!ev) { HCHECK(hipEventRecord(h->xev_go, h->stream)); ev = h->xev_go; }
      HCHECK(hipStreamWaitEvent(h->rf_stream, ev, 0));
      hs = h->rf_stream;
    }
    hipExtLaunchKernelGGL(xheads_out_kernel, dim3(V), dim3(256), 0, hs, nullptr, h->xh_ev[t % 4], 0, (const u32*)hdev, myhead, d.shard_rank,
                          h->xh_host + (size_t)(t % 4) * V * SIM_SREQ_HEAD_WORDS);
    HCHECK(hipGetLastError());
    h->xh_tick[t % 4] = t;
  }
  if (!inl) h->xpending = true;
  return SIM_OK;
}
int sim_exchange_wait(sim_handle* h) {
  if (!h) return SIM_EINVAL;
  if (!h->xcomm) return SIM_ESTATE;
  if (h->xpending) {
    HCHECK(hipEventRecord(h->xev_done, h->xstream));
    HCHECK(hipStreamWaitEvent(h->stream, h->xev_done, 0));
    h->xpending = false;
  }
  return SIM_OK;
}

// Test hook: a shard handle packs its own slab in place WITHOUT a communicator (four handles on one GPU: the test's device copies
// stand in for the exchange and skip the diagonal, like sim_exchange_chunk does)
int sim_t_self_direct(sim_handle* h, int on) {
  if (!h || !h->d.sharded || !h->d.rfan || !h->bound) return SIM_EINVAL;
  h->self_direct = on != 0;
  return SIM_OK;
}
// Test hook (SIM_CF_RANDOM_FANOUT; exported, not declared in the header): the fan-out graph of ANY tick, through the handle's own
// launch path — rf_build with its RfP, its choice of instantiation and its scratch — after both streams have drained; buffer
// tick % 3 then holds that tick's graph and rf_q says so: rf_ready / rf_look_ahead build again whatever the tick needs.
//   which = 0  what the handle builds.  One handle: rcsr[Nl + 1] | rsrc[rcsr[Nl]].  A shard (the sending side), per sender
//              chunk: rsrc[f * Nl / C] | cntb[N] bytes, padded to a word | btot[NB] | xoff[2 V + 2].
//   which = 1  a shard's receiving side as the last sim_step_begin left it, nothing is built: rx_rcsr[Nl + 1] | rx_rsrc[rx_rcsr[Nl]].
// Returns the words written (SIM_ERANGE: more than cap_words).  info: 0 LB, 1 PB, 2 NB, 3 NBh, 4 cap, 5 bcap, 6 wide entries,
// 7 lean rf_rows, 8 NWG, the slab's 9 cnt_u, 10 tot_u, 11 cell_u, 12 slab_u, 13 cap (0 on one handle), and of the build just
// run (a shard: of its last chunk): 14 the largest bucket total, 15 the entries on the overflow list.
int sim_t_rf_graph(sim_handle* h, uint64_t tick, uint32_t which, uint32_t* out, size_t cap_words, uint32_t* info) {
  if (!h || !h->d.rfan || !out || !info || which > 1u || (which == 1u && !h->d.sharded) || h->in_tick) return SIM_EINVAL;
  const Dev& d = h->d;
  const RfP& r = h->rfp;
  const u32 C = d.sharded ? h->rf_C : 1u, spw = h->rf_wide ? RfSpw<u64>::v : RfSpw<u32>::v;
  const u32 set[14] = {r.LB, r.PB, r.NB, r.NBh, r.cap, r.bcap, h->rf_wide ? 1u : 0u, rf_lean(r) ? 1u : 0u, (d.Nl / C + spw - 1u) / spw,
                       d.sharded ? h->rfx.cnt_u : 0u, d.sharded ? h->rfx.tot_u : 0u, d.sharded ? h->rfx.cell_u : 0u,
                       d.sharded ? h->rfx.slab_u : 0u, d.sharded ? h->rfx.cap : 0u};
  memcpy(info, set, sizeof set);
  info[14] = info[15] = 0;
  HCHECK(hipStreamSynchronize(h->rf_stream));
  HCHECK(hipStreamSynchronize(h->stream));
  size_t at = 0;
  auto take = [&](const void* src, size_t words) -> int {  // `words` words of device memory -> out[at ..]
    if (at + words > cap_words) return SIM_ERANGE;
    if (words && hipMemcpy(out + at, src, words * 4u, hipMemcpyDeviceToHost) != hipSuccess) return SIM_EDEVICE;
    at += words;
    return SIM_OK;
  };
  if (which == 1u) {
    if (int rc = take(h->rx_rcsr, (size_t)d.Nl + 1u)) return rc;
    if (int rc = take(h->rx_rsrc, std::min<u32>(out[d.Nl], h->rx_cap))) return rc;
    return (int)at;
  }
  if (int rc = rf_build(h, tick, h->stream)) return rc;
  // (rf_done[tick % 3] is not recorded: both streams were drained above and this build is waited for below, so whatever that event
  // last marked — or nothing — has completed and rf_ready's hipEventQuery on it succeeds without a wait)
  h->rf_q[tick % 3] = tick;
  HCHECK(hipStreamSynchronize(h->stream));
  {  // the counters of the parity the (last) build used: the next build zeroes them
    const u32 par = h->rf_par ^ 1u;
    std::vector<u32> g((size_t)r.NB * RF_GCS);
    HCHECK(hipMemcpy(g.data(), h->rf_gcur[par], g.size() * 4u, hipMemcpyDeviceToHost));
    for (u32 b = 0; b < r.NB; ++b) info[14] = std::max(info[14], g[(size_t)b * RF_GCS]);
    HCHECK(hipMemcpy(&info[15], h->rf_ovf[par], 4u, hipMemcpyDeviceToHost));
  }
  const u32 i = (u32)(tick % 3);
  if (!d.sharded) {
    if (int rc = take(h->rf_rcsr[i], (size_t)d.Nl + 1u)) return rc;
    if (int rc = take(h->rf_rsrc[i], std::min<u32>(out[d.Nl], r.rcap))) return rc;
    return (int)at;
  }
  const size_t per = (size_t)d.f * (d.Nl / C);
  for (u32 c = 0; c < C; ++c) {
    const size_t cw = ((size_t)d.N + 3u) / 4u;
    if (int rc = take(h->rf_rsrc[i] + c * per, per)) return rc;
    if (at + cw > cap_words) return SIM_ERANGE;
    out[at + cw - 1u] = 0;  // (the padding of the count bytes)
    if (hipMemcpy(out + at, h->rf_cntb[i] + (size_t)c * d.N, d.N, hipMemcpyDeviceToHost) != hipSuccess) return SIM_EDEVICE;
    at += cw;
    if (int rc = take(h->rf_btot[i] + (size_t)c * r.NB, r.NB)) return rc;
    if (int rc = take(h->rf_xoff[i] + (size_t)c * (2u * d.V + 2u), 2u * (size_t)d.V + 2u)) return rc;
  }
  return (int)at;
}
// Test hook (host arithmetic only, no device): the fan-out map of `tick` for global node `gid` — its targets and the
// nodes whose packets land on it, both through the general forms the support kernels use.  Returns feff.
int sim_t_fanmap(const sim_config* cfg, uint64_t tick, uint32_t gid, uint32_t* targets, uint32_t* sources) {
  if (!cfg || !targets || !sources || !cfg->vshards || gid >= cfg->n_nodes) return SIM_EINVAL;
  TickP p;
  tickp_make(&p, cfg, tick);
  u32 g = gid / p.M, ll = gid - g * p.M;
  for (u32 k = 0; k < p.feff; ++k) {
    u32 h, t, sg, sl;
    fan_target_g(p, g, ll, k, h, t);
    targets[k] = h * p.M + t;
    fan_source_g(p, p.off[k], p.rot[k], p.rho[k], g, ll, k, sg, sl);
    sources[k] = sg * p.M + sl;
  }
  return (int)p.feff;
}
