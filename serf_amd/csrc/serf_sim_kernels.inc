// serf_sim_kernels.inc — part of the translation unit serf_sim.hip (included from there, in this order; not a header of its own).
// device: every other kernel — API operations, the random fan-out's graph build and packed exchange, push-pull, fills, canonical dumps and digests, statistics, recycling scans, the canonical inbox.
// ------------------------------------------------------------------------------------------------
// operations (user-facing API acting on one node): one thread, a handful of ops per launch
// ------------------------------------------------------------------------------------------------
struct OpBatch {
  u32 n;
  u32 op[8], node[8], a[8], b[8];
  u32 c[8];  // SIM_OP_QUERY: tracker index
  u64 val[8];  // SIM_OP_DELIVER: the record's value
};
__device__ static inline void up_set(const Dev& d, u32 gid, bool up) {
  u32 w = d.upmap[gid >> 5];
  d.upmap[gid >> 5] = up ? (w | (1u << (gid & 31))) : (w & ~(1u << (gid & 31)));
}
__global__ void ops_kernel(Dev d, OpBatch ob, u64 tick, u32 has_alive, u64 qbase, u32 q_timeout) {
  if (threadIdx.x || blockIdx.x) return;
  for (u32 i = 0; i < ob.n; ++i) {
    u32 gid = ob.node[i], op = ob.op[i];
    // ground-truth liveness is replicated on every shard (probes read it)
    if (op == SIM_OP_CRASH) up_set(d, gid, false);
    if (op == SIM_OP_REVIVE || op == SIM_OP_JOIN) up_set(d, gid, true);
    // base.rs:905-930: the QueryResponse is registered before the query goes out (every shard counts its own nodes)
    if (op == SIM_OP_QUERY) d.qtab[ob.c[i]] = make_uint4(ob.a[i], gid, (u32)tick + q_timeout, ob.b[i]);
    if (op == SIM_OP_SET_TAGS) TAGCLASS(d)[gid] = (uint8_t)ob.a[i];  // replicated like liveness: a table the host fills
    if (op == SIM_OP_QRESP) {  // handle_query_response (base.rs:1158-1204): an ack / a response that came in over the byte boundary.
      // Trackers and liveness are replicated; the responder's bit lives on the shard that owns the responder
      const u32 j = ob.a[i] % SIM_QT, from = ob.b[i] & 0xFFFFFFu, which = (ob.b[i] >> 31) ? 0u : 1u;
      const size_t words = ((size_t)d.N + 31) / 32;
      const uint4 t = d.qtab[j];
      if (from >= d.shard0 && from < d.shard0 + d.Nl && up_of(d, gid) && t.x == ob.a[i] && t.y == gid && (u32)tick <= t.z)
        d.qbits[((size_t)j * 2 + which) * words + (from >> 5)] |= 1u << (from & 31);
      continue;
    }
    if (gid < d.shard0 || gid >= d.shard0 + d.Nl) continue;
    u32 l = gid - d.shard0;
    Ctx c{d, l, gid, (u32)tick, qbase};
    Node n;
    node_load(d, l, n);
    node_q_renorm(c, n);  // (the queue through qkeys in place: one thread, any depth — dq_* in serf_sim_state.inc)
    n.dirty = DR0 | DR1 | DR2 | DR3;  // ops are rare: write the whole row back
    bool up = n.flags & SIM_RF_UP, dirty = false;
    u32 a = ob.a[i], b = ob.b[i];
    Ins ins, ins2;  // ins: what the handler queues; ins2: the op's own broadcast, queued after it
    ins.has = ins2.has = ins.wide = ins2.wide = 0;
    switch (op) {
      case SIM_OP_USER_EVENT:  // api.rs:241-299
        if (up) {
          u64 lt = n.eclock;
          n.eclock++;
          uint4* p = ering_ptr(c, lt);
          uint4 e_ = p[0];
          handle_user_event(c, n, a, lt, p, e_, dirty);
          ins_set(ins2, a, wire_meta(SIM_K_EVENT, (b >> 31) ? SIM_F_CC : 0u, b & 0x7FFFFFFFu), lt);
        }
        break;
      case SIM_OP_QUERY:  // base.rs:875-942
        if (up) {
          u64 lt = n.qclock;
          uint4* p = qring_ptr(c, lt);
          uint4 e_ = p[0];
          handle_query(c, n, a, lt, b, p, e_, dirty);
          ins_set(ins2, a, wire_meta(SIM_K_QUERY, b, 48), lt);
        }
        break;
      case SIM_OP_LEAVE:  // api.rs:422-460
        if (up && SIM_RF_STATE(n.flags) == SIM_SERF_ALIVE) {
          n.flags = (n.flags & ~(3u << 1)) | (SIM_SERF_LEAVING << 1);
          u64 lt = n.clock;
          n.clock++;
          uint4* p = view_ptr(c, gid);
          uint4 e_ = p ? p[0] : make_uint4(0, 0, 0, 0);
          handle_leave_intent(c, n, gid, lt, false, p, e_, dirty, ins);
          if (has_alive) ins_set(ins2, gid, wire_meta(SIM_K_LEAVE, 0, 16), lt);
        }
        break;
      case SIM_OP_LEAVE_FINISH:  // api.rs:474-497: memberlist.leave (dead{self, from = self}), state = Left
        if (up && SIM_RF_STATE(n.flags) == SIM_SERF_LEAVING) {
          if (d.swim) {
            uint4* p = view_ptr(c, gid);
            uint4 e_ = p ? p[0] : make_uint4(0, 0, 0, 0);
            swim_dead(c, n, gid, n.inc, gid, wire_meta(SIM_K_DEAD, 0, 32), p, e_, dirty, ins);
          }
          n.flags = (n.flags & ~(3u << 1)) | (SIM_SERF_LEFT << 1);
        }
        break;
      case SIM_OP_JOIN:  // api.rs:318-364
        n.flags |= SIM_RF_UP;
        n.flags = (n.flags & ~(3u << 1)) | (SIM_SERF_ALIVE << 1);
        if (d.swim) {
          uint4* p = view_ptr(c, gid);
          u32 old = SIM_SWIM_ALIVE, accused = n.inc;
          if (p) {
            uint4 e = p[0];
            old = SIM_VB_SWIM(e.w);
            accused = e.z;
            e.w = vb_set_nconf(vb_set_swim(e.w, SIM_SWIM_ALIVE), 0);
            p[0] = e;
          }
          swim_refute(c, n, accused, ins);
          aw_delta(n, -1);
          if (p && (old == SIM_SWIM_DEAD || old == SIM_SWIM_LEFT)) {
            uint4 e = p[0];
            node_join_e(c, n, e, gid);
            p[0] = e;
          }
        }
        broadcast_join(c, n, n.clock, dirty, ins2);
        break;
      case SIM_OP_FORCE_LEAVE:  // base.rs:452-480
        if (up) {
          u64 lt = n.clock;
          uint4* p = view_ptr(c, a);
          uint4 e_ = p ? p[0] : make_uint4(0, 0, 0, 0);
          handle_leave_intent(c, n, a, lt, b != 0, p, e_, dirty, ins);
          if (has_alive) ins_set(ins2, a, wire_meta(SIM_K_LEAVE, b ? SIM_F_PRUNE : 0, 16), lt);
        }
        break;
      case SIM_OP_SET_TAGS:  // api.rs:219-235: memberlist.update_node = next incarnation + an alive broadcast
        if (up && d.swim) {
          swim_refute(c, n, n.inc, ins);
          ins.wmeta |= SIM_F_META;  // the meta differs from the one the previous incarnation carried
          aw_delta(n, -1);  // not an accusation
        }
        break;
      case SIM_OP_CRASH: n.flags &= ~SIM_RF_UP; break;
      case SIM_OP_REVIVE: n.flags |= SIM_RF_UP; break;
      case SIM_OP_PRUNE:  // the end of handle_prune's wait (base.rs:1636-1652): the member goes, whatever it has become
        if (up) {
          uint4* p = view_ptr(c, a);
          if (p) {
            const uint4 e_ = p[0];
            if (e_.w & SIM_VB_KNOWN) erase_member(c, n, p, e_, a);
          }
        }
        break;
      case SIM_OP_SUSPECT:  // the suspicion of a probe that failed last tick on a then slot-less target (swim_probe)
        if (up && d.swim) {
          uint4* p = view_ptr(c, a);
          if (p) {
            uint4 e_ = p[0];
            swim_suspect(c, n, a, e_.z, gid, wire_meta(SIM_K_SUSPECT, 0, 32), p, e_, dirty, ins);
          }
        }
        break;
      case SIM_OP_DELIVER:  // a record from outside the cluster: notify_message (delegate.rs:157-315) / memberlist's own handling
        if (up) {
          u64 val = ob.val[i];
          const bool mute = b & SIM_DELIVER_MUTE;
          b &= SIM_META_WIRE_MASK;
          uint4 r = make_uint4(a, b, (u32)val, (u32)(val >> 32));
          u32 kind = SIM_META_KIND(b);
          u64 vbase = (u64)(uintptr_t)d.view;
          uint4* p = lookup_ptr(c, vbase, (u64)(uintptr_t)d.ering - vbase, (u64)(uintptr_t)d.qring - vbase, kind, a, val, slot_load(d, kind, a));
          uint4 e_ = p ? p[0] : make_uint4(0, 0, 0, 0);
          if (mute) {  // out of a PushPull message: merge_remote_state (delegate.rs:495-552) — the handlers' verdicts are dropped, a
                       // refutation (broadcast_join: `ins`, set inside the handler) is not
            if (kind == SIM_K_LEAVE) (void)handle_leave_intent(c, n, a, val, false, p, e_, dirty, ins);
            else if (kind == SIM_K_JOIN) (void)handle_join_intent(c, n, a, val, p, e_, dirty);
            else if (kind == SIM_K_EVENT) (void)handle_user_event(c, n, a, val, p, e_, dirty);
          } else dispatch(c, n, r, p, e_, dirty, ins);
        }
        break;
      case SIM_OP_WITNESS:  // a PushPull message's clocks (delegate.rs:466-480)
        if (up) {
          if (a == 0) witness(n, n.clock, ob.val[i], DR0);
          else if (a == 1) witness(n, n.eclock, ob.val[i], DR1);
          else witness(n, n.qclock, ob.val[i], DR1);
        }
        break;
      default: break;
    }
    if (ins.has) node_q_insert(c, n, ins.key, ins.wmeta, ins.val);
    if (ins2.has) node_q_insert(c, n, ins2.key, ins2.wmeta, ins2.val);
    node_store(d, l, n);
    __threadfence();  // the next op of this batch may touch the same node
  }
}

// ------------------------------------------------------------------------------------------------
// SIM_CF_RANDOM_FANOUT — memberlist's kRandomNodes (App. B.2; oracle rf_draw / rf_group): the tick's fan-out graph
// ------------------------------------------------------------------------------------------------
// Every node draws its `fanout` gossip targets uniformly over the other nodes, without replacement: a function of (seed,
// tick, node) alone, so the graph of tick t can be built before — or while — anything else of tick t runs, and any kernel
// that needs a target draws it again instead of reading it (a handful of mix64 per node against 16 bytes of HBM).
// What the tick kernel needs of it: for every receiver the row rsrc[rcsr[t] .. rcsr[t + 1]) of the (sender, slot) pairs
// p = 4 l + k that drew it, p ascending: the oracle hands a node its packets in (sender, slot) order.  That is a sort of
// f * N pairs by (target, p); the keys are uniform, so it is done as a two-level bucket sort written for this job (no
// library on the per-tick path), two launches per tick:
//   rf_scatter  every workgroup draws the targets of its SPW senders, counts them per level-1 bucket (= 2^LB consecutive
//               targets) in LDS, reserves its share of every bucket's REGION with one global atomic per (workgroup, bucket),
//               lays the pairs down in LDS bucket by bucket and writes them out from there: l1[b * bcap + ...], runs of
//               ~ 4 SPW / NB pairs stored by consecutive lanes.  The regions have a
//               fixed capacity bcap (mean 4 * 2^LB + 12 sigma: uniform draws never fill one); what does not fit all the
//               same goes onto an overflow list.  Any order inside a bucket will do: the order that counts is restored by
//               rank, not by stability — so the result does not depend on who won which atomic.
//   rf_rows     one workgroup per bucket: its place in the output = the sum of the totals of the buckets before it; an LDS
//               counting sort by target -> the bucket's part of rcsr; every pair ranks itself among the ~ f pairs of its row
//               (p ascending) -> its place in rsrc, laid down in LDS and written out as one run.  Pairs and targets stay in
//               registers between the passes.  A bucket that does not fit the LDS tables (never with uniform draws; forced
//               by the tests through SERF_RF_CAP) ranks straight from global memory.
struct RfP {
  u64 rb;       // rng_base(seed, STREAM_RFAN, tick)
  u32 N, Nl, shard0, feff, f;
  u32 Ns;       // senders whose targets are drawn: the handle's own Nl (global id shard0 + l; pair ids p = 4 * l + slot are local)
  u32 rcap;     // entries rsrc holds
  u32 LB, NB;   // level-1 buckets: ranges of 2^LB consecutive targets — NB = ceil(Nl / 2^LB) of them; on a shard (r5: the sort is
                // the SENDING side's, over the targets of the shard's own senders anywhere in the cluster) NBh = ceil(M / 2^LB) per
                // destination shard, NB = V * NBh: a bucket never straddles two shards
  u32 V, M, NBh;  // destination shards, their size, buckets per destination (one handle that holds every node: 1, N, NB)
  u32 lfirst;     // the first sender of this build (a shard's sender chunk c: c * M / C; else 0), Ns senders from there
  u32 PB;       // bits of a pair id p = 4 l + k; a scattered entry is (target - bucket start) << PB | p — 32 bits when they fit
  u32 NWG;      // workgroups of rf_scatter (RfSpw senders each)
  u32 cap;      // pairs rf_rows can rank in LDS (a multiple of RFR, at most RF_EPT * RFR)
  u32 bcap;     // pairs a bucket's region of l1 holds
  u32 ocap;     // entries of the overflow list
};
#define RFB 1024          // threads of an rf_scatter workgroup
#define RF_GCS 1u         // stride of the buckets' fill counters in words (a line each — 32 — made the atomics slower: 55.7 vs 47.6 us, profiles/r04_experiments.md)
// senders of an rf_scatter workgroup, by entry width: their pairs are staged in LDS (6 / 10 bytes a pair) and leave as runs of
// 4 SPW / NB entries — 4096 senders: 102 KiB of LDS with 32-bit entries; 64-bit entries (above 4 Mi nodes) take 2048
#ifndef RF_SPW32
#define RF_SPW32 4096u
#endif
template <typename E> struct RfSpw { static constexpr u32 v = sizeof(E) == 4 ? RF_SPW32 : 2048u; };
#ifndef RFR
#define RFR 512           // threads of an rf_rows workgroup
#endif
#ifndef RF_LB_MAX
#define RF_LB_MAX 13u     // at most 8192 rows per level-1 bucket (64 KiB of rf_rows' LDS; one handle that holds every node stays at 11 or below)
#endif
#define RF_EPT 24u        // pairs one thread of rf_rows keeps in registers: cap <= RF_EPT * RFR
// exclusive prefix over the 64 lanes of a wave (`total` = the sum)
__device__ static inline u32 wave_excl_scan(u32 v, u32& total) {
  u32 x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    u32 y = (u32)__shfl_up((int)x, o, 64);
    if ((threadIdx.x & 63u) >= (u32)o) x += y;
  }
  total = (u32)__shfl((int)x, 63, 64);
  return x - v;
}
// gcur[NB]: pairs in each bucket so far (zero at launch: rf_rows of the build before zeroed it); ovf: [0] = entries, then (bucket, entry) pairs
// LDS of rf_scatter (dynamic): cnt[NB] | lst[NB] | cur[NB] | stage: E[f * SPW] | stb: u16[f * SPW]
template <typename E>
static inline size_t rf_scatter_lds(const RfP& r) { return (((size_t)3u * r.NB * 4u + 7u) & ~(size_t)7u) + (size_t)SIM_MAX_FANOUT * RfSpw<E>::v * (sizeof(E) + 2u); }
template <typename E>
__global__ __launch_bounds__(RFB) void rf_scatter_kernel(RfP r, u32* gcur, E* l1, E* ovf) {
  constexpr u32 SPW = RfSpw<E>::v;
  extern __shared__ u32 rf_lds[];
  // cnt: the workgroup's pairs per bucket, then its base in the bucket's region; lst: where the bucket's run starts in the
  // staging area; cur: cursors.  The pairs are laid down in LDS bucket by bucket and leave as runs: consecutive lanes store
  // consecutive entries of a region (scattered 4-byte stores straight from the drawing lanes cost 30 of this kernel's 48 us)
  u32 *cnt = rf_lds, *lst = cnt + r.NB, *cur = lst + r.NB;
  E* stage = reinterpret_cast<E*>(reinterpret_cast<char*>(rf_lds) + (((size_t)3u * r.NB * 4u + 7u) & ~(size_t)7u));
  uint16_t* stb = reinterpret_cast<uint16_t*>(stage + (size_t)SIM_MAX_FANOUT * SPW);
  __shared__ u32 wsum[RFB / 64u];
  for (u32 b = threadIdx.x; b < 3u * r.NB; b += RFB) rf_lds[b] = 0;
  __syncthreads();
  const u32 l0 = blockIdx.x * SPW;
  u32 tg[SPW / RFB][SIM_MAX_FANOUT], nc[SPW / RFB];
#pragma unroll
  for (u32 j = 0; j < SPW / RFB; ++j) {
    const u32 l = l0 + j * RFB + threadIdx.x;  // the sender: local index lfirst + l, global id shard0 + lfirst + l
    nc[j] = l < r.Ns ? rf_draw(r.rb, r.shard0 + r.lfirst + l, r.N, r.feff, tg[j]) : 0u;
#pragma unroll
    for (u32 k = 0; k < SIM_MAX_FANOUT; ++k)
      if (k < nc[j]) {  // from here on a target is (bucket << 16 | offset in the bucket): the bucket never straddles two shards
        const u32 t = tg[j][k], h = r.V == 1u ? 0u : t / r.M, tl = t - h * r.M;
        const u32 b = h * r.NBh + (tl >> r.LB);
        tg[j][k] = (b << 16) | (tl & ((1u << r.LB) - 1u));
        atomicAdd(&cnt[b], 1u);
      }
  }
  __syncthreads();
  {  // exclusive prefix of the counts (every thread a stretch of buckets), and the workgroup's share of every region
    const u32 per = (r.NB + RFB - 1u) / RFB, b0 = threadIdx.x * per, b1 = min(b0 + per, r.NB);
    u32 sum = 0;
    for (u32 b = b0; b < b1; ++b) sum += cnt[b];
    u32 wtot;
    u32 run = wave_excl_scan(sum, wtot);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = wtot;
    __syncthreads();
    for (u32 w = 0; w < (threadIdx.x >> 6); ++w) run += wsum[w];
    for (u32 b = b0; b < b1; ++b) {
      const u32 c = cnt[b];
      lst[b] = run;
      run += c;
      cnt[b] = c ? atomicAdd(&gcur[(size_t)b * RF_GCS], c) : 0u;
    }
  }
  __syncthreads();
#pragma unroll
  for (u32 j = 0; j < SPW / RFB; ++j) {
    const u32 l = l0 + j * RFB + threadIdx.x;
#pragma unroll
    for (u32 k = 0; k < SIM_MAX_FANOUT; ++k) {
      if (k < nc[j]) {  // (a slot without a target — fewer other nodes than the fan-out — is in nobody's row)
        const u32 b = tg[j][k] >> 16, at = lst[b] + atomicAdd(&cur[b], 1u);
        stage[at] = ((E)(tg[j][k] & 0xFFFFu) << r.PB) | (E)(4u * (r.lfirst + l) + k);
        stb[at] = (uint16_t)b;
      }
    }
  }
  __syncthreads();
  u32 total = 0;
  for (u32 w = 0; w < RFB / 64u; ++w) total += wsum[w];
  for (u32 i = threadIdx.x; i < total; i += RFB) {  // any order inside a bucket will do (rf_rows ranks)
    const u32 b = stb[i], at = cnt[b] + (i - lst[b]);
    const E e = stage[i];
    if (at < r.bcap) l1[(size_t)b * r.bcap + at] = e;
    else {
      const u32 o = atomicAdd(reinterpret_cast<u32*>(ovf), 1u);
      if (o < r.ocap) { ovf[1u + 2u * o] = (E)b; ovf[2u + 2u * o] = e; }
    }
  }
}
// LDS of rf_rows (dynamic): cnt[R + 1] | cur[R] | rowp[cap]
static inline size_t rf_rows_lds(const RfP& r) { return ((size_t)(2u << r.LB) + 1u + r.cap) * 4u + 16u; }
// (r6) EPT = pairs a thread keeps in registers, PERMAX = rows a thread scans in the prefix: the loops over them are fully unrolled and
// predicated, and the build's instructions are what it costs the step (profiles/r06_experiments.md) — the launch picks the lean
// instantiation <11, 2> when the bucket's capacity and width allow (one handle at 1 Mi nodes: 5 632 pairs = the mean and 16 sigma, 1 024 rows), the general one
// <EPT, 2^RF_LB_MAX / RFR> otherwise
template <typename E, u32 EPT, u32 PERMAX>
__global__ __launch_bounds__(RFR) void rf_rows_kernel(RfP r, u32* gcur, u32* gcur_next, const E* l1, E* ovf, E* ovf_next, u32* rcsr, u32* rsrc, uint8_t* cntb, u32* btot, u32* xflag) {
  // (cntb != null: the SENDING side's sort of a shard — instead of row starts, one count byte per target of every destination
  // shard, cntb[h * M + t], and the bucket's total, btot[b]: what travels with the packets; rsrc = the sorted pair ids)
  extern __shared__ u32 rf_lds[];
  const u32 R = 1u << r.LB;
  u32 *cnt = rf_lds, *cur = cnt + R + 1u, *rowp = cur + R;
  __shared__ u32 wtot[RFR / 64u], s_base;
  const u32 b = blockIdx.x, n = gcur[(size_t)b * RF_GCS], nreg = min(n, r.bcap);
  const u32 hb = b / r.NBh, t0 = (b - hb * r.NBh) << r.LB, nrows = min(R, r.M - t0);
  const E pmask = ((E)1 << r.PB) - (E)1;
  // the bucket's place in the output: behind everything the buckets before it hold
  {
    u32 part = 0;
    for (u32 i = threadIdx.x; i < b; i += RFR) part += gcur[(size_t)i * RF_GCS];
    u32 wsum;
    (void)wave_excl_scan(part, wsum);
    if ((threadIdx.x & 63u) == 0) wtot[threadIdx.x >> 6] = wsum;
  }
  for (u32 i = threadIdx.x; i <= R; i += RFR) cnt[i] = 0;
  for (u32 i = threadIdx.x; i < R; i += RFR) cur[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 sum = 0;
    for (u32 w = 0; w < RFR / 64u; ++w) sum += wtot[w];
    s_base = sum;
    gcur_next[(size_t)b * RF_GCS] = 0;  // the next build's counters start from zero (it runs behind this one, on the same stream)
    if (b == 0) *reinterpret_cast<u32*>(ovf_next) = 0;
  }
  // entry i of the bucket: the first nreg in its region of l1, the rest on the overflow list (any order)
  auto entry = [&](u32 i) __attribute__((always_inline)) -> E {
    if (i < nreg) return l1[(size_t)b * r.bcap + i];
    u32 seen = 0, tot = min(*reinterpret_cast<const u32*>(ovf), r.ocap);
    for (u32 j = 0; j < tot; ++j)
      if (ovf[1u + 2u * j] == (E)b) { if (seen == i - nreg) return ovf[2u + 2u * j]; ++seen; }
    return (E)0;  // (cannot happen: the list holds the rest of this bucket — it cannot run full, sim_create sizes it for every pair)
  };
  const bool fits = n <= r.cap;
  u32 pv[EPT];
  uint16_t tv[EPT];
#pragma unroll
  for (u32 j = 0; j < EPT; ++j) {
    const u32 i = threadIdx.x + j * RFR;
    pv[j] = NOSLOT; tv[j] = 0;
    if (fits && i < n) {
      const E e = entry(i);
      pv[j] = (u32)(e & pmask);
      tv[j] = (uint16_t)(e >> r.PB);
      atomicAdd(&cnt[tv[j]], 1u);
    }
  }
  if (!fits)
    for (u32 i = threadIdx.x; i < n; i += RFR) atomicAdd(&cnt[(u32)(entry(i) >> r.PB)], 1u);
  __syncthreads();
  const u32 base = s_base;
  {  // exclusive prefix over the bucket's rows: every thread R / RFR consecutive ones (R <= 4096; a smaller R: one each)
    const u32 per = (R + RFR - 1u) / RFR, i0 = threadIdx.x * per;
    u32 v[PERMAX], sum = 0;
#pragma unroll
    for (u32 j = 0; j < PERMAX; ++j) { v[j] = (j < per && i0 + j < R) ? cnt[i0 + j] : 0u; sum += v[j]; }
    u32 wsum, run = wave_excl_scan(sum, wsum);
    if ((threadIdx.x & 63u) == 0) wtot[threadIdx.x >> 6] = wsum;  // (everybody is past the sync behind the first use of wtot)
    __syncthreads();
    for (u32 w = 0; w < (threadIdx.x >> 6); ++w) run += wtot[w];
#pragma unroll
    for (u32 j = 0; j < PERMAX; ++j)
      if (j < per && i0 + j < R) { cnt[i0 + j] = run; run += v[j]; }
    if (threadIdx.x == RFR - 1u) cnt[R] = run;
  }
  __syncthreads();
  if (cntb) {
    for (u32 i = threadIdx.x; i < nrows; i += RFR) {
      const u32 c = cnt[i + 1u] - cnt[i];
      if (c > 255u) atomicOr(xflag, 1u);  // (a node drawn by more than 255 of one shard's senders in one tick)
      cntb[(size_t)hb * r.M + t0 + i] = (uint8_t)min(c, 255u);
    }
    if (threadIdx.x == 0) btot[b] = n;
  } else {
    for (u32 i = threadIdx.x; i < nrows; i += RFR) rcsr[t0 + i] = base + cnt[i];
    if (b == r.NB - 1u && threadIdx.x == 0) rcsr[r.Nl] = base + n;
  }
  if (fits) {
#pragma unroll
    for (u32 j = 0; j < EPT; ++j)
      if (pv[j] != NOSLOT) rowp[cnt[tv[j]] + atomicAdd(&cur[tv[j]], 1u)] = pv[j];
    __syncthreads();
#pragma unroll
    for (u32 j = 0; j < EPT; ++j) {
      if (pv[j] != NOSLOT) {
        const u32 lo = cnt[tv[j]], hi = cnt[tv[j] + 1u];
        u32 rank = 0;
        for (u32 q = lo; q < hi; q += 2u) {  // two entries a turn (the second may be the next row's first, or the slack word behind the last: masked)
          const u32 a = rowp[q], b = rowp[q + 1u];
          rank += (a < pv[j] ? 1u : 0u) + ((q + 1u < hi && b < pv[j]) ? 1u : 0u);
        }
        tv[j] = (uint16_t)(lo + rank);  // (its place in the bucket: below 2^16, the row is not needed any more)
      }
    }
    __syncthreads();  // the rows have been read: the sorted bucket goes into the same LDS, then out as one run
#pragma unroll
    for (u32 j = 0; j < EPT; ++j)
      if (pv[j] != NOSLOT) rowp[tv[j]] = pv[j];
    __syncthreads();
    for (u32 i = threadIdx.x; i < n; i += RFR)
      if (base + i < r.rcap) rsrc[base + i] = rowp[i];  // (a shard: more packets than rsrc has room for — mean + 12 sigma — cannot happen)
  } else {  // the bucket does not fit the tables: rank every pair against the whole bucket, straight from global memory
    for (u32 i = threadIdx.x; i < n; i += RFR) {
      const E e = entry(i);
      u32 rank = 0;
      for (u32 j = 0; j < n; ++j) {
        const E q = entry(j);
        rank += ((q >> r.PB) == (e >> r.PB) && (q & pmask) < (e & pmask)) ? 1u : 0u;
      }
      const u32 at = base + cnt[(u32)(e >> r.PB)] + rank;
      if (at < r.rcap) rsrc[at] = (u32)(e & pmask);
    }
  }
}
// ---- SIM_CF_RANDOM_FANOUT on a shard (r5): the packed exchange (include/serf_sim.h SIM_XCHG_PACKED) ----------------------------
// A packet goes to ANY node of the cluster.  The packets stay in their senders' cells (as on one GPU); per tick every shard
//   * sorts the (target, sender, slot) triples of its OWN senders by global target (rf_scatter / rf_rows above, two ticks ahead on
//     the build stream): rsrc = the sorted pair ids p = 4 l + k, cntb = one count byte per target of every destination shard,
//     btot = the buckets' totals, xoff = where every destination's pairs start (rfx_soff_kernel);
//   * PACKS, behind the tick kernel, the packets bound for shard h into slab h of the send buffer in that order (rfx_pack_kernel:
//     pair -> sender's cell 0 and its map word -> the packet's pages, one scattered 64-byte read per packet — the read the
//     receiver does on one GPU), the count bytes and bucket totals of h next to them (rfx_meta_kernel);
//   * after the round's all-to-all turns the V slabs it received into the tick's CSR (rfx_index_kernel): a node's row = V runs,
//     source shards ascending = senders ascending; an entry of rsrc = the packet's cell in the receive buffer, so the tick
//     kernel reads it exactly as it reads a sender's cell 0 (map word: "this cell, n pages"; pages adjacent: Dev::NC = 1).
// A slab, in 64-byte units: header {packets, overflow flag, tick} | count bytes [M] | bucket totals [NBh] u32 | cells [cap * PG].
struct RfxL {  // the layout of one slab (the same on every shard of a run)
  u32 V, C, M, NBh, LB, PG, cap;  // C sender chunks per tick: slab (c, h) of the send buffer = what chunk c's senders address to shard h
  u32 cnt_u, tot_u, cell_u, slab_u;  // offsets of the three sections and the slab's size, in 64-byte units
};
static RfxL rfx_layout(u32 V, u32 C, u32 M, u32 NBh, u32 LB, u32 PG, u32 f) {
  RfxL x;
  x.V = V; x.C = C; x.M = M; x.NBh = NBh; x.LB = LB; x.PG = PG;
  x.cap = serf_rf_slab_cap(f, M / C, V);
  x.cnt_u = 1u;
  x.tot_u = x.cnt_u + (M + 63u) / 64u;
  x.cell_u = x.tot_u + (NBh + 15u) / 16u;
  x.slab_u = x.cell_u + x.cap * PG;
  return x;
}
// where every destination's pairs start in the sorted list (xoff[0 .. V]); xoff[V + 1 + h] = 1 when slab h cannot hold them
__global__ void rfx_soff_kernel(RfxL x, const u32* btot, u32* xoff, u32* xflag) {  // one workgroup of 256: a wave per destination at a time
  __shared__ u32 part[64];
  const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (u32 h = wave; h < x.V; h += blockDim.x >> 6) {
    u32 sum = 0;
    for (u32 j = lane; j < x.NBh; j += 64u) sum += btot[(size_t)h * x.NBh + j];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += (u32)__shfl_xor((int)sum, o, 64);
    if (lane == 0) part[h] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 run = 0;
    for (u32 h = 0; h < x.V; ++h) {
      xoff[h] = run;
      run += part[h];
      xoff[x.V + 1u + h] = part[h] > x.cap ? 1u : 0u;
      if (part[h] > x.cap) atomicOr(xflag, 2u);
    }
    xoff[x.V] = run;
  }
}
// the slabs' headers, count bytes and bucket totals (what the receiver makes its rows from)
// (`self_slab`, r6: when the library issues the round's exchange itself, the slab a shard addresses to ITSELF — slab `self_h` — is
// written straight into its place in the receive buffer and never travels; null: every slab goes into the send buffer)
__global__ void rfx_meta_kernel(RfxL x, const uint8_t* cntb, const u32* btot, const u32* xoff, u32 tick, uint4* send, u32 self_h, uint4* self_slab) {
  // (r6) 16 bytes a thread where the layout allows — M a multiple of 16: the count bytes of destination h start at cntb + h * M, their
  // section of the slab is 64-byte aligned — (one byte a thread cost 24 us a tick for 1 MiB of count bytes)
  const bool wide = (x.M & 15u) == 0u;
  const size_t cu = wide ? (size_t)(x.M >> 4) : (size_t)x.M;  // units of the count section: uint4 or bytes
  const size_t per = cu + (size_t)x.NBh + 16u;                // ... then one unit per bucket total, then the header's 16 words
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < per * x.V; i += (size_t)gridDim.x * blockDim.x) {
    const u32 h = (u32)(i / per);
    const size_t o = i - (size_t)h * per;
    uint8_t* slab = reinterpret_cast<uint8_t*>((self_slab && h == self_h) ? self_slab : send + (size_t)h * x.slab_u * 4u);
    if (o < cu) {
      if (wide) reinterpret_cast<uint4*>(slab + (size_t)x.cnt_u * 64u)[o] = reinterpret_cast<const uint4*>(cntb + (size_t)h * x.M)[o];
      else slab[(size_t)x.cnt_u * 64u + o] = cntb[(size_t)h * x.M + o];
    } else if (o < cu + (size_t)x.NBh) {
      const size_t w = o - cu;
      reinterpret_cast<u32*>(slab + (size_t)x.tot_u * 64u)[w] = btot[(size_t)h * x.NBh + w];
    } else {
      const u32 i4 = (u32)(o - cu - (size_t)x.NBh);
      const u32 n = xoff[h + 1u] - xoff[h], over = xoff[x.V + 1u + h];
      reinterpret_cast<u32*>(slab)[i4] = i4 == 0u ? min(n, x.cap) : i4 == 1u ? over : i4 == 2u ? tick : 0u;
    }
  }
}
// (r6) the heads of the tick's slot-less suspicion lists, as the round's exchange delivered them (sim_exchange_chunk), into pinned
// host memory: workgroup w = rank w's head — this rank's own straight from its list —, the count and the pairs the list holds
// (a word when it is empty: every tick but a few), written by the kernel itself: no copy command, no other stream
__global__ void xheads_out_kernel(const u32* dev, const u32* mine, u32 rank, u32* host) {
  const u32 w = blockIdx.x;
  const u32* src = w == rank ? mine : dev + (size_t)w * SIM_SREQ_HEAD_WORDS;
  u32* dst = host + (size_t)w * SIM_SREQ_HEAD_WORDS;
  const u32 n = src[0], words = 1u + 2u * min(n, (u32)SIM_SREQ_HEAD_PAIRS);
  for (u32 i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
}
// pair i of the sorted list -> its packet, copied into its place in the slab of its destination: four lanes per packet, one
// 16-byte quarter each, consecutive pairs -> consecutive cells (dense 64-byte writes); the fourth quarter of a packet's first
// cell is its map word ("this cell, n pages" — or all 0xFF: nothing was sent / the packet was lost).  The sender's cell 0 is
// asked for whole, on spec, before its map word (its fourth quarter) is known — 99 % of the packets sit there: ONE scattered line per
// packet, and RFX_U packets per quad in flight at once; a packet in another of its sender's cells, or a further page, is a second fetch.
#define RFX_U 4u
__global__ void rfx_pack_kernel(RfxL x, const u32* rsrc, const u32* xoff, const uint4* cells, u32 Nl, uint4* send, u32 self_h, uint4* self_slab) {
  const u32 xV = x.V, xcap = x.cap, xslab = x.slab_u, xcell = x.cell_u, xPG = x.PG;  // (the lambda below must not take the argument's address: scratch)
  const u32 total = xoff[xV];
  const u32 q = threadIdx.x & 3u;
  const size_t quads = ((size_t)gridDim.x * blockDim.x) >> 2, quad = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  auto place = [&](size_t i, u32 p, const v4u c0) __attribute__((always_inline)) {
    const u32 mw = (u32)__shfl((int)c0.x, (int)((threadIdx.x & 63u) | 3u), 64);  // the quad's fourth lane holds the map word
    u32 h = 0;
    while (h + 1u < xV && xoff[h + 1u] <= (u32)i) ++h;
    const u32 pos = (u32)i - xoff[h];
    if (i < total && pos < xcap) {  // (a full slab: its header says so and the step fails)
      const u32 l = p >> 2, k = p & 3u;
      const u32 jb = (mw >> (8u * k)) & 0xFFu;
      const u32 pages = jb == 0xFFu ? 0u : (jb & 3u) + 1u;
      uint4* dst = ((self_slab && h == self_h) ? self_slab : send + (size_t)h * xslab * 4u) + ((size_t)xcell + (size_t)pos * xPG) * 4u;
      for (u32 pg = 0; pg < xPG; ++pg) {
        v4u v = {0u, 0u, 0u, 0u};
        if (q == 3u) v.x = pg == 0u ? (pages ? (0xFFFFFF00u | (pages - 1u)) : 0xFFFFFFFFu) : 0xFFFFFFFFu;
        else if (pg < pages) v = ((jb >> 2) + pg == 0u) ? c0 : *reinterpret_cast<const v4u*>(&cells[((size_t)((jb >> 2) + pg) * Nl + l) * RF_CELL_U4 + q]);
        *reinterpret_cast<v4u*>(&dst[(size_t)pg * 4u + q]) = v;
      }
    }
  };
  static_assert(RFX_U == 4u, "four packets per quad in flight");
  // (the quad's four packets of a sweep are `quads` pairs apart: for each of them the wave's 16 quads read 16 consecutive pair
  // ids and write 16 consecutive cells — 1 KiB runs)
  for (size_t i0 = quad; i0 < total; i0 += quads * RFX_U) {
    const size_t i1 = i0 + quads, i2 = i1 + quads, i3 = i2 + quads;
    const u32 pa = rsrc[i0], pb = i1 < total ? rsrc[i1] : 0u, pc = i2 < total ? rsrc[i2] : 0u, pd = i3 < total ? rsrc[i3] : 0u;
    const v4u* cv = reinterpret_cast<const v4u*>(cells);
    const v4u ca = cv[(size_t)(pa >> 2) * RF_CELL_U4 + q], cb = cv[(size_t)(pb >> 2) * RF_CELL_U4 + q];
    const v4u cc = cv[(size_t)(pc >> 2) * RF_CELL_U4 + q], cd = cv[(size_t)(pd >> 2) * RF_CELL_U4 + q];
    place(i0, pa, ca); place(i1, pb, cb); place(i2, pc, cc); place(i3, pd, cd);
  }
}
// the receiving side: one workgroup per bucket of 2^LB targets — the bucket's place in every source's slab and in the rows is
// the sum of the totals before it (they travelled with the packets); inside it, prefix sums over the count bytes
#define RFX_T 256u
// LDS (dynamic): rs[R] u32 — where the next entry of every row goes | cb[V][R] u8 — the bucket's count bytes of every source, staged
// once (one coalesced pass over global memory; everything after it reads LDS) | bef[V] u32 — what the buckets before this one hold
static inline size_t rfx_index_lds(const RfxL& x) { return ((size_t)4u << x.LB) + ((size_t)(x.V * x.C) << x.LB) + (size_t)x.V * x.C * 4u + 16u; }
__global__ __launch_bounds__(RFX_T) void rfx_index_kernel(RfxL x, const uint4* recv, u32 Nl, u32 rcap, u32* rcsr, u32* rsrc, u32* xflag) {
  extern __shared__ u32 rfx_lds[];
  __shared__ u32 wsum[RFX_T / 64u];
  // (V below: the SOURCES, in the order of their senders — shard g's chunks 0 .. C - 1, then shard g + 1's —; source q sits in slab
  // (q % C) * shards + q / C of the receive buffer)
  const u32 R = 1u << x.LB, V = x.V * x.C, b = blockIdx.x, t0 = b << x.LB, nrows = min(R, x.M - t0);
  u32* rs = rfx_lds;
  uint8_t* cb = reinterpret_cast<uint8_t*>(rs + R);
  u32* bef = reinterpret_cast<u32*>(cb + ((size_t)V << x.LB));
  const u32 per = (R + RFX_T - 1u) / RFX_T, i0 = threadIdx.x * per, i1 = min(i0 + per, nrows);
  auto slab_of = [&](u32 q) __attribute__((always_inline)) -> u32 { return (q % x.C) * x.V + q / x.C; };
  auto slab = [&](u32 q) __attribute__((always_inline)) -> const uint8_t* { return reinterpret_cast<const uint8_t*>(recv + (size_t)slab_of(q) * x.slab_u * 4u); };
  auto block_excl = [&](u32 v, u32& total) __attribute__((always_inline)) -> u32 {  // exclusive prefix over the workgroup's threads
    u32 wt, run = wave_excl_scan(v, wt);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = wt;
    __syncthreads();
    total = 0;
    for (u32 w = 0; w < RFX_T / 64u; ++w) { if (w < (threadIdx.x >> 6)) run += wsum[w]; total += wsum[w]; }
    return run;
  };
  for (u32 g = threadIdx.x; g < V; g += RFX_T) bef[g] = 0;
  __syncthreads();
  // one pass over global memory: the count bytes of this bucket from every source (4 at a time: the sections are 64-byte aligned,
  // a bucket starts at a multiple of 2^LB >= 4, the padding behind a ragged last bucket is the section's own), the totals of the
  // buckets before it, and — one workgroup — the headers: a sender whose slab ran full says so there
  for (u32 g = 0; g < V; ++g) {
    const u32* src = reinterpret_cast<const u32*>(slab(g) + (size_t)x.cnt_u * 64u + t0);
    u32* dst = reinterpret_cast<u32*>(cb + ((size_t)g << x.LB));
    for (u32 w = threadIdx.x; w < (nrows + 3u) / 4u; w += RFX_T) dst[w] = src[w];
    const u32* tot = reinterpret_cast<const u32*>(slab(g) + (size_t)x.tot_u * 64u);
    u32 part = 0;
    for (u32 j = threadIdx.x; j < b; j += RFX_T) part += tot[j];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += (u32)__shfl_xor((int)part, o, 64);
    if ((threadIdx.x & 63u) == 0 && part) atomicAdd(&bef[g], part);
    if (threadIdx.x == 0 && b == 0) {
      const u32* hd = reinterpret_cast<const u32*>(slab(g));
      if (hd[1] != 0u || hd[0] > x.cap) atomicOr(xflag, 4u);
    }
  }
  __syncthreads();
  u32 before = 0;
  for (u32 g = 0; g < V; ++g) before += bef[g];
  // the rows' starts: the prefix of the rows' lengths (all sources), behind everything the buckets before this one hold
  u32 mine = 0;
  for (u32 i = i0; i < i1; ++i)
    for (u32 g = 0; g < V; ++g) mine += cb[((size_t)g << x.LB) + i];
  u32 tot_rows;
  u32 run = block_excl(mine, tot_rows) + before;
  for (u32 i = i0; i < i1; ++i) {
    u32 c = 0;
    for (u32 g = 0; g < V; ++g) c += cb[((size_t)g << x.LB) + i];
    rs[i] = run;
    rcsr[t0 + i] = run;
    run += c;
  }
  if (b == gridDim.x - 1u && threadIdx.x == RFX_T - 1u) rcsr[Nl] = before + tot_rows;
  if (threadIdx.x == 0 && before + tot_rows > rcap) atomicOr(xflag, 8u);  // (more packets than rsrc has room for: mean + 12 sigma)
  // source by source: the entries of a row's run from source g = the cells of g's slab from the row's offset on
  for (u32 g = 0; g < V; ++g) {
    const uint8_t* cg = cb + ((size_t)g << x.LB);
    u32 sum = 0;
    for (u32 i = i0; i < i1; ++i) sum += cg[i];
    u32 ts;
    u32 off = block_excl(sum, ts) + bef[g];
    const u32 cell0 = slab_of(g) * x.slab_u + x.cell_u;  // (64-byte units from the start of the receive buffer)
    for (u32 i = i0; i < i1; ++i) {
      const u32 c = cg[i];
      u32 at = rs[i];
      for (u32 k = 0; k < c; ++k, ++at, ++off)
        if (at < rcap) rsrc[at] = (cell0 + off * x.PG) << 2;
      rs[i] = at;
    }
  }
}
// gossip_to_the_dead_time with random fan-out (oracle tick_node): bit k of the node's skip byte = its view, as the tick begins,
// says the target it drew for slot k has been dead / left for longer than that.  Its own launch, only when the option is on.
__global__ void rf_skip_kernel(Dev d, TickP tp, RfP r, const uint4* base) {
  for (size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * blockDim.x) {
    u32 ch[SIM_MAX_FANOUT], m = 0;
    const u32 nc = rf_draw(r.rb, d.shard0 + (u32)l, r.N, r.feff, ch);
    for (u32 k = 0; k < nc; ++k) {
      const u32 key = SEL4(k, ch[0], ch[1], ch[2], ch[3]), a = d.slot_of[key];
      uint4 e = a == NOSLOT ? base[(size_t)key * 2] : d.view[(size_t)a * d.Nl + l];
      u32 sw = SIM_VB_SWIM(e.w);
      if ((e.w & SIM_VB_KNOWN) && (sw == SIM_SWIM_DEAD || sw == SIM_SWIM_LEFT) && ((((u32)tp.tick - SIM_VB_STAMP(e.w)) & STAMP_MASK) > d.gttd)) m |= 1u << k;
    }
    d.skipmask[l] = (uint8_t)m;
  }
}
// gossip_to_the_dead_time (App. B.2; oracle gossip_skips): for every node and fan-out slot, does the node's view — as it is when
// the tick begins — say that the packet's target has been dead / left for longer than that?  Its own launch, ahead of
// the tick kernel and only when the option is on: the tick kernel then reads one byte per node.
__global__ void gossip_skip_kernel(Dev d, TickP tp, const uint4* base) {
  for (size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * blockDim.x) {
    u32 gid = d.shard0 + (u32)l, g = gid / tp.M, ll = gid - g * tp.M, m = 0;
    for (u32 k = 0; k < tp.feff; ++k) {
      u32 hh, tt;
      fan_target_g(tp, g, ll, k, hh, tt);
      u32 target = hh * tp.M + tt, a = d.slot_of[target];
      uint4 e = a == NOSLOT ? base[(size_t)target * 2] : d.view[(size_t)a * d.Nl + l];
      u32 sw = SIM_VB_SWIM(e.w);
      if ((e.w & SIM_VB_KNOWN) && (sw == SIM_SWIM_DEAD || sw == SIM_SWIM_LEFT) && ((((u32)tp.tick - SIM_VB_STAMP(e.w)) & STAMP_MASK) > d.gttd)) m |= 1u << k;
    }
    d.skipmask[l] = (uint8_t)m;
  }
}
// SIM_CF_JOIN_SYNC (oracle join_sync): memberlist.join = a push-pull with the peer — the joining node adopts the view of a
// running node of its own shard.  One block: the partner is picked by thread 0, the entries are copied in parallel, the
// suspicion timers of the adopted entries are listed in walk order, chunk by chunk.
__global__ void join_sync_kernel(Dev d, u32 n_slots, u32 gid, u32 peer, u32 tick) {
  __shared__ u32 s_partner;
  __shared__ u32 s_flag[BLOCK];  // view slot + 1 of an adopted entry that is suspect, 0 otherwise
  __shared__ u32 s_nt, s_next, s_ovf;
  const u32 M = d.M, base = (gid / M) * M, l = gid - d.shard0;
  if (!threadIdx.x) {
    u32 partner = NOSLOT;
    for (u32 i = 0; i < M && partner == NOSLOT; ++i) {
      u32 cand = base + (peer % M + i) % M;
      if (cand != gid && up_of(d, cand)) partner = cand;
    }
    s_partner = partner;
    s_nt = 0; s_next = 0xFFFFFFFFu; s_ovf = 0;
  }
  __syncthreads();
  if (s_partner == NOSLOT) return;
  const u32 lp = s_partner - d.shard0;
  uint16_t* sp = reinterpret_cast<uint16_t*>(&d.R4[2 * (size_t)l]);
  if (threadIdx.x < SIM_S) sp[threadIdx.x] = 0;
  for (u32 w0 = 0; w0 < n_slots; w0 += BLOCK) {
    u32 wi = w0 + threadIdx.x;
    u32 flag = 0, deadline = 0;
    if (wi < n_slots) {
      u32 a = d.walk[wi];
      uint4* e = d.view + ((size_t)a * d.Nl + l);
      const uint4* pe = d.view + ((size_t)a * d.Nl + lp);
      uint4 h = pe[0];
      if (d.subject_of[a] == gid) {  // its own entry stays its own
        uint4 mine = e[0];
        if (h.z > mine.z) { mine.z = h.z; e[0] = mine; }
      } else {
        e[0] = h;
        e[d.vtail] = pe[d.vtail];
        if ((h.w & SIM_VB_KNOWN) && SIM_VB_SWIM(h.w) == SIM_SWIM_SUSPECT) {  // the adopted suspicion keeps running here
          flag = a + 1;
          deadline = tick - ((tick - SIM_VB_STAMP(h.w)) & STAMP_MASK) + d.T[SIM_VB_NCONF(h.w)];
        }
      }
    }
    s_flag[threadIdx.x] = flag;
    __syncthreads();
    if (!threadIdx.x)
      for (u32 i = 0; i < BLOCK; ++i)
        if (s_flag[i]) {
          if (s_nt == SIM_S) s_ovf++;
          else sp[s_nt++] = (uint16_t)s_flag[i];
        }
    __syncthreads();
    // earliest deadline over the TRACKED timers: thread 0 cannot see the deadlines, so every flagged thread checks whether
    // its slot made it into the list
    if (flag) {
      bool tracked = false;
      for (u32 j = 0; j < SIM_S; ++j) tracked |= sp[j] == (uint16_t)flag;
      if (tracked) atomicMin(&s_next, deadline);
    }
    __syncthreads();
  }
  if (!threadIdx.x) {
    uint4 r0 = d.R0[l], r1 = d.R1[l], r2 = d.R2[l], r3 = d.R3[l];
    const uint4 p0 = d.R0[lp], p1 = d.R1[lp], p2 = d.R2[lp], p3 = d.R3[lp];
    u32 a_me = d.slot_of[gid];
    u32 pst = SIM_STATUS_NONE, mst = SIM_STATUS_NONE, pknown = 0, mknown = 0;
    if (a_me != NOSLOT) {
      uint4 pm = d.view[(size_t)a_me * d.Nl + lp], mm = d.view[(size_t)a_me * d.Nl + l];
      if (pm.w & SIM_VB_KNOWN) { pst = SIM_VB_STATUS(pm.w); pknown = 1u; }
      if (mm.w & SIM_VB_KNOWN) { mst = SIM_VB_STATUS(mm.w); mknown = 1u; }
    }
    r3.y = s_next == 0xFFFFFFFFu ? 0u : s_next;  // susp_next
    r3.w = p3.w;         // reap_next
    r1.w = p1.w - pknown + mknown;  // n_known: the partner's, corrected for the joiner's own entry (the partner may have reaped the joiner; oracle join_sync)
    r2.x = p2.x - (pst == SIM_STATUS_FAILED ? 1u : 0u) + (mst == SIM_STATUS_FAILED ? 1u : 0u);
    r2.y = p2.y - (pst == SIM_STATUS_LEFT ? 1u : 0u) + (mst == SIM_STATUS_LEFT ? 1u : 0u);
    r2.w += s_ovf;
    u64 c = (u64)r0.x | ((u64)r0.y << 32), ec = (u64)r0.z | ((u64)r0.w << 32), qc = (u64)r1.x | ((u64)r1.y << 32);
    u64 pc = (u64)p0.x | ((u64)p0.y << 32), pec = (u64)p0.z | ((u64)p0.w << 32), pqc = (u64)p1.x | ((u64)p1.y << 32);
    if (pc > 0 && pc - 1 >= c) c = pc;       // witness(remote - 1): delegate.rs:466-480
    if (pec > 0 && pec - 1 >= ec) ec = pec;
    if (pqc > 0 && pqc - 1 >= qc) qc = pqc;
    r0 = make_uint4((u32)c, (u32)(c >> 32), (u32)ec, (u32)(ec >> 32));
    r1.x = (u32)qc; r1.y = (u32)(qc >> 32);
    d.R0[l] = r0; d.R1[l] = r1; d.R2[l] = r2; d.R3[l] = r3;
  }
}

// ------------------------------------------------------------------------------------------------
// deep_queue_kernel (r6) — phase 2 of the tick for the nodes the tick kernel left alone: a queue of more than HQ entries (or one
// that this tick's parked broadcasts could take there).  Behind every tick-kernel launch, one node of the launch's deep list per
// lane: the node's sort keys — up to SIM_Q — are staged in LDS ([SIM_Q][64] words: a lane's column, conflict-free for the
// lanes that walk in step), the parked broadcasts are queued in arrival order, the QueueChecker runs on its ticks, `fanout`
// packets are drained under the byte budget and written where the tick kernel would have written them (its own cells and map
// word; the cells of the exchange buffer on a shard), keys and row go back.  A node that ends the tick with at most HQ entries is
// made shallow again (payloads moved into slots below HQ).  Same results as the oracle's tick_node on a queue of SIM_Q records;
// none of this runs at the benchmark's headline load (the list is empty: the grid's waves read one word and leave).
// ------------------------------------------------------------------------------------------------
struct SlotsL {  // the payload slots of the packet being drained, in drain order: a lane's column of bytes in LDS
  uint8_t* lds;  // [SIM_PKT_RECORDS_MAX][TBLOCK]
  u32 tid;
  __device__ void set(u32 i, u32 v) const { lds[i * TBLOCK + tid] = (uint8_t)v; }
  __device__ u32 get(u32 i) const { return lds[i * TBLOCK + tid]; }
};
__global__ __launch_bounds__(TBLOCK) void deep_queue_kernel(Dev d, TickP tp, u32 cur, u32* seen_host) {
  __shared__ u32 lds_k[SIM_Q * TBLOCK];
  __shared__ uint8_t lds_s[SIM_MAX_FANOUT][SIM_PKT_RECORDS_MAX * TBLOCK];
  const u32 tid = threadIdx.x;
  const u32 total = d.deep_cnt[d.deep_par];
  if (blockIdx.x == 0 && tid == 0) {
    d.deep_cnt[d.deep_par ^ 1u] = 0;  // the next launch's list starts empty (its last reader finished a launch ago)
    if (total) { d.deep_cnt[2] = max(d.deep_cnt[2], total); d.deep_cnt[3] += 1u; if (seen_host) *seen_host = max(*seen_host, total); }
  }
  const KeysL kl{lds_k, tid};
  for (u32 it = blockIdx.x * TBLOCK + tid; it < total; it += gridDim.x * TBLOCK) {
    const uint2 ent = d.deep_list[(size_t)d.deep_par * d.Nl + it];
    const u32 l = ent.x, npend = ent.y, gid = d.shard0 + l;
    const uint4 r1 = d.R1[l];
    uint4 r2 = d.R2[l];  // (written by the tick kernel: n_failed, n_left, overflow as the handlers left them)
    DQ q;
    dq_open(d, l, r2, q);
    const u32 cnt_in = q.cnt;
    for (u32 g = 0; g < SIM_Q / 4u; ++g) {
      uint4 k4 = make_uint4(KEMPTY, KEMPTY, KEMPTY, KEMPTY);
      if (4u * g < cnt_in) k4 = d.qkeys[(size_t)g * d.Nl + l];
      kl.set(4u * g, k4.x); kl.set(4u * g + 1u, k4.y); kl.set(4u * g + 2u, k4.z); kl.set(4u * g + 3u, k4.w);
    }
    if (q.next_seq > 1023u - 64u) dq_renorm(kl, q);
    for (u32 i = 0; i < npend; ++i) {
      const uint4 pq = d.pend[(size_t)i * d.Nl + l];
      dq_insert(d, l, kl, q, pq.x, pq.y, (u64)pq.z | ((u64)pq.w << 32));
    }
    if (d.queue_check_interval && ((u32)tp.tick + (gid >> 6)) % d.queue_check_interval == 0) {
      u32 mx = d.max_queue_depth;
      if (d.min_queue_depth > 0) mx = max(2u * r1.w, d.min_queue_depth);
      dq_queue_check(kl, q, mx);
    }
    const u32 limit = d.retransmit_mult * digits10(r1.w);
    u32 skipm = d.gttd ? (u32)d.skipmask[l] : 0u;
    if (d.rfan && d.N < 256u) {
      u32 ch[SIM_MAX_FANOUT];
      const u32 nc = rf_draw(tp.rfan_base, gid, d.N, tp.feff, ch);
      skipm |= (0xFu << nc) & 0xFu;
    }
    // ---- drain: `fanout` packets, their payload slots in LDS ----
    u32 cn[SIM_MAX_FANOUT] = {0, 0, 0, 0};
#pragma unroll
    for (u32 k = 0; k < SIM_MAX_FANOUT; ++k) {
      if (k >= tp.feff) break;
      const SlotsL so{lds_s[k], tid};
      const u32 c = dq_round(kl, q, limit, d.P, so);
      const bool lost = (tp.loss_u32 && (u32)(mix64(tp.loss_base ^ ((u64)gid * 4u + k)) >> 32) < tp.loss_u32) || ((skipm >> k) & 1u);
      cn[k] = lost ? 0u : c;
    }
    // ---- the packets: every distinct one once (the tick kernel's rule: same slots in the same positions = the same packet) ----
    const bool local = !d.sharded || d.rfan;  // the packets stay in the sender's cells (a shard of the random fan-out packs them afterwards)
    const u32 cu4 = d.rfan ? RF_CELL_U4 : PK_U4;
    u32 jmap = 0xFFFFFFFFu, used_pg = 0;
    u32 first[SIM_MAX_FANOUT] = {0, 0, 0, 0};
    bool isnew[SIM_MAX_FANOUT] = {false, false, false, false};
#pragma unroll
    for (u32 k = 0; k < SIM_MAX_FANOUT; ++k) {
      if (k >= tp.feff || cn[k] == 0u) continue;
      u32 jenc = 0xFFu;
      bool nw = true;
      for (u32 p = 0; p < k && nw; ++p) {
        if (cn[p] != cn[k]) continue;
        bool same = true;
        for (u32 i = 0; i < cn[k]; ++i) same &= lds_s[p][i * TBLOCK + tid] == lds_s[k][i * TBLOCK + tid];
        if (same) { jenc = (jmap >> (8u * p)) & 0xFFu; nw = false; }
      }
      if (nw) {
        const u32 np = (cn[k] + SIM_P - 1u) / SIM_P;
        first[k] = used_pg; isnew[k] = true;
        jenc = (used_pg << 2) | (np - 1u);
        used_pg += np;
      }
      jmap = (jmap & ~(0xFFu << (8u * k))) | (jenc << (8u * k));
    }
    u32 g = tp.V == 1 ? 0u : gid / tp.M, ll = gid - g * tp.M;
#pragma unroll
    for (u32 k = 0; k < SIM_MAX_FANOUT; ++k) {
      if (k >= tp.feff) break;
      uint4* dbase;
      size_t pstride;
      u32 pages;
      if (local) {
        if (!isnew[k]) continue;
        dbase = d.obox[cur ^ 1u] + ((size_t)first[k] * d.Nl + l) * cu4;
        pstride = (size_t)d.Nl * cu4;
        pages = (cn[k] + SIM_P - 1u) / SIM_P;
      } else {  // a shard of the bijection: the cell of the exchange buffer T_k(l) reads (oracle xcell); every page is written, empty ones as zeros
        u32 h, t;
        fan_target_g(tp, g, ll, k, h, t);
        const u32 s0 = ((ll % tp.blk) / tp.sub), r = (t % tp.blk) % tp.sub;
        dbase = d.xsend + ((((size_t)s0 * tp.V + h) * d.fp + (size_t)k * d.PG) * tp.sub + r) * PK_U4;
        pstride = (size_t)tp.sub * PK_U4;
        pages = d.PG;
      }
      for (u32 pg = 0; pg < pages; ++pg) {
        u32 wk[SIM_P] = {0, 0, 0, 0}, wl[SIM_P] = {0, 0, 0, 0}, wh[SIM_P] = {0, 0, 0, 0};
#pragma unroll
        for (u32 p = 0; p < SIM_P; ++p) {
          const u32 idx = 4u * pg + p;
          if (idx < cn[k]) {
            const uint4 rec = d.qpay[(size_t)lds_s[k][idx * TBLOCK + tid] * d.Nl + l];
            wire_pack(rec, wk[p], wl[p], wh[p]);
          }
        }
        uint4* dst = dbase + (size_t)pg * pstride;
        dst[0] = make_uint4(wk[0], wk[1], wk[2], wk[3]); dst[1] = make_uint4(wl[0], wl[1], wl[2], wl[3]); dst[2] = make_uint4(wh[0], wh[1], wh[2], wh[3]);
        if (d.rfan) dst[3] = make_uint4(jmap, 0u, 0u, 0u);
      }
    }
    if (local && !d.rfan) d.omap[cur ^ 1u][l] = jmap;
    if (d.rfan && jmap == 0xFFFFFFFFu) d.obox[cur ^ 1u][(size_t)l * RF_CELL_U4 + 3u] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
    // ---- back to shallow when the queue fits the hot keys again: payloads into slots below HQ ----
    if (q.cnt <= HQ && (q.used >> HQ) != 0ull) {
      for (u32 i = 0; i < q.cnt; ++i) {
        const u32 ki = kl.get(i), sl = ki & QK_SLOT_MASK;
        if (sl < HQ) continue;
        const u32 ns = (u32)__ffsll((unsigned long long)(~q.used & 0xFFFFull)) - 1u;
        d.qpay[(size_t)ns * d.Nl + l] = d.qpay[(size_t)sl * d.Nl + l];
        q.used = (q.used & ~(1ull << sl)) | (1ull << ns);
        kl.set(i, (ki & ~QK_SLOT_MASK) | ns);
      }
    }
    const u32 hi = max(cnt_in, q.cnt);
    for (u32 g4 = 0; g4 < SIM_Q / 4u; ++g4)
      if (4u * g4 < hi) d.qkeys[(size_t)g4 * d.Nl + l] = make_uint4(kl.get(4u * g4), kl.get(4u * g4 + 1u), kl.get(4u * g4 + 2u), kl.get(4u * g4 + 3u));
    r2.z = dq_close(d, l, q);
    r2.w = q.overflow;
    d.R2[l] = r2;
  }
}

// ------------------------------------------------------------------------------------------------
// push-pull anti-entropy (memberlist pushPull, App. B.6; SerfDelegate::local_state / merge_remote_state,
// serf-core/src/serf/delegate.rs:386-554) — SIMSPEC §2.10, oracle pp_round/pp_pair/pp_merge.
// One lane per synchronising pair; a batch holds 1/PP_GROUPS of all pairs, so the launch fills the chip
// and happens once per (scaled interval / PP_GROUPS) ticks: off the per-tick critical path.
// ------------------------------------------------------------------------------------------------
#define PP_GROUPS 8u
// What one side of a push-pull ships to the other (memberlist's node states + SerfDelegate::local_state,
// delegate.rs:386-425): the three clocks, the 16-byte heads of the view entries in walk (subject) order, the event
// ring.  The partner's copy is read either in place (it lives on this shard) or from a flat record a remote shard
// exported (sim_pp_export): [0] {clock, event_clock} [1] {query_clock, 0} [2 .. 2+ns) heads [..] (X + Bev) x {head, tail}: the overflow rows, then the buckets.
// (`bmap`: the event ring's planes that have memory — LazyPlanes, serf_sim_host.inc; the buckets beyond them are empty)
struct PPLocal {
  const Dev& d;
  u32 lr, bmap;
  __device__ void clocks(u64& c, u64& e, u64& q) const {
    uint4 r0 = d.R0[lr], r1 = d.R1[lr];
    c = (u64)r0.x | ((u64)r0.y << 32); e = (u64)r0.z | ((u64)r0.w << 32); q = (u64)r1.x | ((u64)r1.y << 32);
  }
  __device__ uint4 head(u32 wi) const { return d.view[(size_t)d.walk[wi] * d.Nl + lr]; }
  __device__ uint4 bucket_head(u32 idx) const { return idx < bmap ? d.ering[(size_t)idx * d.Nl + lr] : make_uint4(0, 0, 0, 0); }
  __device__ uint4 bucket_tail(u32 idx) const { return d.ering[d.etail + (size_t)idx * d.Nl + lr]; }  // (asked for behind a non-empty head only)
  // overflow row j of the partner's event ring (rows in front of bucket 0; always mapped)
  __device__ uint4 ovf_head(u32 j) const { return (d.ering - (size_t)(d.X - j) * d.Nl)[lr]; }
  __device__ uint4 ovf_tail(u32 j) const { return (d.ering - (size_t)(d.X - j) * d.Nl)[d.etail + lr]; }
};
struct PPRecord {
  const uint4* rec;
  u32 ns;
  __device__ void clocks(u64& c, u64& e, u64& q) const {
    uint4 r0 = rec[0], r1 = rec[1];
    c = (u64)r0.x | ((u64)r0.y << 32); e = (u64)r0.z | ((u64)r0.w << 32); q = (u64)r1.x | ((u64)r1.y << 32);
  }
  __device__ uint4 head(u32 wi) const { return rec[2 + wi]; }
  u32 X;  // the record holds the ring's X overflow rows, then its buckets
  __device__ uint4 bucket_head(u32 idx) const { return rec[2 + ns + 2 * (size_t)(X + idx)]; }
  __device__ uint4 bucket_tail(u32 idx) const { return rec[2 + ns + 2 * (size_t)(X + idx) + 1]; }
  __device__ uint4 ovf_head(u32 j) const { return rec[2 + ns + 2 * (size_t)j]; }
  __device__ uint4 ovf_tail(u32 j) const { return rec[2 + ns + 2 * (size_t)j + 1]; }
};
// local <- remote: memberlist mergeState, then merge_remote_state(is_join = false)
template <class Remote>
__device__ static void pp_merge(const Dev& d, const TickP& tp, u32 ll, const Remote& rm) {
  Ctx c{d, ll, d.shard0 + ll, (u32)tp.tick, tp.query_base};
  Node n;
  node_load(d, ll, n);
  node_q_renorm(c, n);
  const uint4 zero = make_uint4(0, 0, 0, 0);
  bool dirty = false;
  if (d.swim) {  // alive as alive, left as dead{from = node}, suspect and dead as suspect
#pragma unroll 1
    for (u32 wi = 0; wi < tp.n_slots; ++wi) {
      u32 a = d.walk[wi];
      uint4 re = rm.head(wi);
      if (!(re.w & SIM_VB_KNOWN)) continue;
      node_q_renorm(c, n);  // a merge can queue one broadcast per view slot
      u32 subj = d.subject_of[a], sw = SIM_VB_SWIM(re.w), inc = re.z;
      uint4* p = view_slot_ptr(c, a);
      uint4 e = p[0];
      Ins ins;
      ins.has = ins.wide = 0;
      if (sw == SIM_SWIM_ALIVE) swim_alive(c, n, subj, inc, wire_meta(SIM_K_ALIVE, 0, 64), p, e, dirty, ins);
      else if (sw == SIM_SWIM_LEFT) swim_dead(c, n, subj, inc, subj, wire_meta(SIM_K_DEAD, 0, 32), p, e, dirty, ins);
      else swim_suspect(c, n, subj, inc, c.gid, wire_meta(SIM_K_SUSPECT, 0, 32), p, e, dirty, ins);
      if (ins.has) node_q_insert(c, n, ins.key, ins.wmeta, ins.val);
    }
  }
  u64 rclock, reclock, rqclock;
  rm.clocks(rclock, reclock, rqclock);
  if (rclock > 0) witness(n, n.clock, rclock - 1, DR0);     // delegate.rs:466-480
  if (reclock > 0) witness(n, n.eclock, reclock - 1, DR0);
  if (rqclock > 0) witness(n, n.qclock, rqclock - 1, DR1);
#pragma unroll 1
  for (u32 pass = 0; pass < 2; ++pass) {  // left members first (at status_ltime + 1), then the join intents
#pragma unroll 1
    for (u32 wi = 0; wi < tp.n_slots; ++wi) {
      u32 a = d.walk[wi];
      uint4 re = rm.head(wi);
      if (!(re.w & SIM_VB_KNOWN)) continue;
      bool left = SIM_VB_STATUS(re.w) == SIM_STATUS_LEFT;
      if (left != (pass == 0)) continue;
      if (left) node_q_renorm(c, n);
      u32 subj = d.subject_of[a];
      uint4* p = view_slot_ptr(c, a);
      uint4 e = p[0];
      Ins ins;
      ins.has = ins.wide = 0;
      if (left) handle_leave_intent(c, n, subj, E_LTIME(re) + 1, false, p, e, dirty, ins);  // delegate.rs:495-512
      else handle_join_intent(c, n, subj, E_LTIME(re), p, e, dirty);                        // delegate.rs:515-526
      if (ins.has) node_q_insert(c, n, ins.key, ins.wmeta, ins.val);                        // a refutation
    }
  }
#pragma unroll 1
  for (u32 idx = 0; idx < d.Bev; ++idx) {  // replay the remote event buffer: delegate.rs:540-552
    uint4 b0 = rm.bucket_head(idx);
    if (!b0.z) continue;
    uint4 b1 = b0.w ? rm.bucket_tail(idx) : zero;
    u64 lt = E_LTIME(b0);
    u32 keys[SIM_C] = {b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int k = 0; k < (int)SIM_C; ++k) {
      if (!keys[k]) break;
      uint4* p = ering_ptr(c, lt);
      uint4 e_ = p[0];
      handle_user_event(c, n, keys[k], lt, p, e_, dirty);
    }
    if (keys[SIM_C - 1]) {  // a full bucket continues in its overflow rows, in row order (= push order)
#pragma unroll 1
      for (u32 j = 0; j < d.X; ++j) {
        const uint4 h = rm.ovf_head(j);
        if (!h.x) break;
        if (h.x != idx + 1u) continue;
        const uint4 t = h.w ? rm.ovf_tail(j) : zero;
        const u32 ok[SIM_C] = {h.z, h.w, t.x, t.y, t.z, t.w};
#pragma unroll
        for (int k = 0; k < (int)SIM_C; ++k) {
          if (!ok[k]) break;
          uint4* p = ering_ptr(c, lt);
          uint4 e_ = p[0];
          handle_user_event(c, n, ok[k], lt, p, e_, dirty);
        }
      }
    }
  }
  node_store(d, ll, n);
}
// The pairs of a batch: the tick's matching {sigma_N^-1(2 pi), sigma_N^-1(2 pi + 1)} over ALL N nodes — memberlist's
// pushPull picks any peer (App. B.6), whichever shard it lives on — restricted to class pi mod PP_GROUPS.  The node
// with the even sigma value merges first, then the other merges its updated state.  This kernel: every shard local.
__global__ void pushpull_kernel(Dev d, TickP tp, u32 cls, u32 n_pairs, u32 bmap) {
  u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_pairs) return;
  u32 pi = cls + j * PP_GROUPS;
  if (2 * (u64)pi + 1 >= tp.N) return;
  u32 la = sigma_g_inv(tp, 2 * pi), lb = sigma_g_inv(tp, 2 * pi + 1);
  if (!up_of(d, la) || !up_of(d, lb)) return;  // a TCP exchange needs both ends
  pp_merge(d, tp, la, PPLocal{d, lb, bmap});
  pp_merge(d, tp, lb, PPLocal{d, la, bmap});
}
// sharded runs (host-planned, sim_pp_*): the in-shard pairs ...
__global__ void pp_local_kernel(Dev d, TickP tp, const u32* la, const u32* lb, u32 n) {
  u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  pp_merge(d, tp, la[j], PPLocal{d, lb[j], d.Bev});  // (a shard's rings are whole)
  pp_merge(d, tp, lb[j], PPLocal{d, la[j], d.Bev});
}
// ... a handful of pairs handed over by value (the Reconnector's attempts of a tick: pairwise disjoint, `a` merges first) ...
struct PairBatch { u32 n; u32 a[8], b[8]; };
__global__ void pp_pairs_kernel(Dev d, TickP tp, PairBatch pb, u32 bmap) {
  u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= pb.n) return;
  pp_merge(d, tp, pb.a[j], PPLocal{d, pb.b[j], bmap});
  pp_merge(d, tp, pb.b[j], PPLocal{d, pb.a[j], bmap});
}
// ... the records this shard ships (one block per record: `ns` view heads + the event ring) ...
__global__ void pp_export_kernel(Dev d, const u32* list, u32 ns, uint4* out, size_t rec_u4) {
  u32 l = list[blockIdx.x];
  uint4* o = out + (size_t)blockIdx.x * rec_u4;
  for (size_t i = threadIdx.x; i < rec_u4; i += blockDim.x) {
    uint4 v;
    if (i == 0) v = d.R0[l];
    else if (i == 1) { uint4 r1 = d.R1[l]; v = make_uint4(r1.x, r1.y, 0, 0); }
    else if (i < 2 + (size_t)ns) v = d.view[(size_t)d.walk[i - 2] * d.Nl + l];
    else {
      size_t k = i - 2 - ns;
      v = d.ering0[((k & 1) ? d.etail : 0) + (k >> 1) * d.Nl + l];  // (rows: the overflow rows, then the buckets)
    }
    o[i] = v;
  }
}
// ... and the merges from the records it received
__global__ void pp_cross_kernel(Dev d, TickP tp, const u32* list, u32 n, const uint4* recs, size_t rec_u4) {
  u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  pp_merge(d, tp, list[j], PPRecord{recs + (size_t)j * rec_u4, tp.n_slots, d.X});
}

// ------------------------------------------------------------------------------------------------
// support kernels: fills, canonical forms, digest, members, convergence, stats
// ------------------------------------------------------------------------------------------------
__global__ void fill_u32(u32* p, size_t n, u32 v) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
__global__ void fill_u4(uint4* p, size_t n, uint4 v) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
// column a of the view := the subject's baseline entry
__global__ void fill_view_col(uint4* view, size_t tail, size_t Nl, u32 a, uint4 e0, uint4 e1) {
  for (size_t l = blockIdx.x * (size_t)blockDim.x + threadIdx.x; l < Nl; l += (size_t)gridDim.x * blockDim.x) {
    view[(size_t)a * Nl + l] = e0;
    view[tail + (size_t)a * Nl + l] = e1;
  }
}
// the per-subject baseline table stays entry-interleaved ([N][2]): it is read by probes and status queries only
__global__ void fill_base(uint4* base, size_t n, uint4 e0, uint4 e1) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    base[i * 2] = e0;
    base[i * 2 + 1] = e1;
  }
}
// canonical (interleaved, 32-byte) form of `count` entries starting at entry `first` of a split array, and back
__global__ void canon_entries_kernel(const uint4* arr, size_t tail, size_t first, size_t count, uint4* out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    out[i * 2] = arr[first + i];
    out[i * 2 + 1] = arr[tail + first + i];
  }
}
__global__ void uncanon_entries_kernel(uint4* arr, size_t tail, size_t first, size_t count, const uint4* in) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    arr[first + i] = in[i * 2];
    arr[tail + first + i] = in[i * 2 + 1];
  }
}
// keep d.walk sorted by subject: shift [pos, count) up by one, put slot a at pos (one thread; slot allocation is rare)
__device__ static inline void walk_insert(u32* walk, u32 count, u32 pos, u32 a) {
  for (u32 i = count; i > pos; --i) walk[i] = walk[i - 1];
  walk[pos] = a;
}
// A subject takes view slot a: its column of the view := the subject's baseline entry, the slot joins the walk order, the
// two slot maps point at each other.  ONE launch (it used to be four, 4 - 8 us of stream time each, in front of the tick of
// every operation that names a new subject).
__global__ void slot_alloc_kernel(uint4* view, size_t tail, size_t Nl, u32 a, uint4 e0, uint4 e1, u32* walk, u32 count, u32 pos,
                                  u32* slot_of_x, u32* subject_of_a, u32 subject) {
  if (!blockIdx.x && !threadIdx.x) {
    walk_insert(walk, count, pos, a);
    *slot_of_x = a;
    *subject_of_a = subject;
  }
  for (size_t l = blockIdx.x * (size_t)blockDim.x + threadIdx.x; l < Nl; l += (size_t)gridDim.x * blockDim.x) {
    view[(size_t)a * Nl + l] = e0;
    view[tail + (size_t)a * Nl + l] = e1;
  }
}
__global__ void fill_iota(u32* p, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = (u32)i;
}
__global__ void init_dense_self(Dev d) {  // new_in's synthetic notify_join(local): self known, Alive @ 0
  for (size_t l = blockIdx.x * (size_t)blockDim.x + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * blockDim.x) {
    u32 gid = d.shard0 + (u32)l;
    d.view[(size_t)gid * d.Nl + l] = make_uint4(0, 0, 0, 1u | (SIM_STATUS_ALIVE << 1));
  }
}

// canonical sim_row (12 x u64 words) of node l
#define ROW_W 14  // u64 words of a canonical sim_row
static_assert(sizeof(sim_row) == ROW_W * 8, "canonical row");
__device__ static inline void canon_row(const Dev& d, size_t l, u64 (&w)[ROW_W]) {
  uint4 r0 = d.R0[l], r1 = d.R1[l], r2 = d.R2[l], r3 = d.R3[l], r4 = d.R4[2 * l], r4b = d.R4[2 * l + 1], r5 = d.R5[l];
  w[0] = (u64)r0.x | ((u64)r0.y << 32);
  w[1] = (u64)r0.z | ((u64)r0.w << 32);
  w[2] = (u64)r1.x | ((u64)r1.y << 32);
  w[3] = (u64)r5.x | ((u64)r5.y << 32);
  w[4] = (u64)r5.z | ((u64)r5.w << 32);
  w[5] = (u64)r1.z | ((u64)r3.x << 32);              // flags, inc
  w[6] = (u64)r1.w | ((u64)r2.x << 32);              // n_known, n_failed
  w[7] = (u64)r2.y | ((u64)(r2.z & 0x7FFFu) << 32);  // n_left, next_seq
  w[8] = (u64)r2.w | ((u64)r3.y << 32);              // overflow, susp_next
  w[9] = (u64)r3.z | ((u64)r3.w << 32);              // awareness, reap_next
  w[10] = (u64)r4.x | ((u64)r4.y << 32);
  w[11] = (u64)r4.z | ((u64)r4.w << 32);
  w[12] = (u64)r4b.x | ((u64)r4b.y << 32);
  w[13] = (u64)r4b.z | ((u64)r4b.w << 32);
}
// entries in node l's queue (R2.z: the slot mask of a shallow node, or the flag that says it is in Dev::qused)
__device__ static inline u32 q_count(const Dev& d, size_t l, u32 r2z) { return (r2z & QDEEP) ? (u32)__popcll(d.qused[l]) : (u32)__popc(r2z >> 16); }
// canonical sim_record i (drain order) of node l
__device__ static inline uint4 canon_qrec(const Dev& d, size_t l, u32 i, u32 cnt) {
  if (i >= cnt) return make_uint4(0u, SIM_META_EMPTY, 0u, 0u);
  uint4 kq = d.qkeys[(size_t)(i >> 2) * d.Nl + l];
  u32 k = (i & 3) == 0 ? kq.x : (i & 3) == 1 ? kq.y : (i & 3) == 2 ? kq.z : kq.w;
  uint4 pay = d.qpay[(size_t)(k & QK_SLOT_MASK) * d.Nl + l];
  return make_uint4(pay.x, ((k >> QK_SLOT_BITS) << 8) | (pay.y & 0xFFu), pay.z, pay.w);
}
__global__ void canon_rows_kernel(Dev d, u64* out) {
  for (size_t l = blockIdx.x * (size_t)blockDim.x + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * blockDim.x) {
    u64 w[ROW_W];
    canon_row(d, l, w);
    for (int i = 0; i < ROW_W; ++i) out[l * ROW_W + i] = w[i];
  }
}
__global__ void canon_queue_kernel(Dev d, uint4* out) {
  for (size_t l = blockIdx.x * (size_t)blockDim.x + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * blockDim.x) {
    u32 cnt = q_count(d, l, d.R2[l].z);
    for (u32 i = 0; i < SIM_Q; ++i) out[l * SIM_Q + i] = canon_qrec(d, l, i, cnt);
  }
}

// ---- checkpoint / resume: canonical image -> physical layout ----------------------------------------
__global__ void restore_rows_kernel(Dev d, const u64* in /* [Nl][ROW_W] canonical sim_row */) {
  for (size_t l = blockIdx.x * (size_t)blockDim.x + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * blockDim.x) {
    const u64* w = in + l * ROW_W;
    u32 used = d.R2[l].z & 0xFFFF8000u;  // slot mask and depth flag: set by restore_queue_kernel, which runs first
    d.R0[l] = make_uint4((u32)w[0], (u32)(w[0] >> 32), (u32)w[1], (u32)(w[1] >> 32));
    d.R1[l] = make_uint4((u32)w[2], (u32)(w[2] >> 32), (u32)w[5], (u32)w[6]);
    d.R2[l] = make_uint4((u32)(w[6] >> 32), (u32)w[7], ((u32)(w[7] >> 32) & 0x7FFFu) | used, (u32)w[8]);
    d.R3[l] = make_uint4((u32)(w[5] >> 32), (u32)(w[8] >> 32), (u32)w[9], (u32)(w[9] >> 32));
    d.R4[2 * l] = make_uint4((u32)w[10], (u32)(w[10] >> 32), (u32)w[11], (u32)(w[11] >> 32));
    d.R4[2 * l + 1] = make_uint4((u32)w[12], (u32)(w[12] >> 32), (u32)w[13], (u32)(w[13] >> 32));
    d.R5[l] = make_uint4((u32)w[3], (u32)(w[3] >> 32), (u32)w[4], (u32)(w[4] >> 32));
  }
}
__global__ void restore_queue_kernel(Dev d, const uint4* in /* [Nl][Q] canonical sim_record, drain order */) {
  for (size_t l = blockIdx.x * (size_t)blockDim.x + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * blockDim.x) {
    u32 cnt = 0;
    u32* kw = reinterpret_cast<u32*>(d.qkeys);
    for (u32 i = 0; i < SIM_Q; ++i) {
      uint4 r = in[l * SIM_Q + i];
      u32 k = KEMPTY;
      if (r.y != SIM_META_EMPTY) {
        k = ((r.y >> 8) << QK_SLOT_BITS) | i;  // payload slot = rank
        d.qpay[(size_t)i * d.Nl + l] = make_uint4(r.x, r.y & SIM_META_WIRE_MASK, r.z, r.w);
        cnt++;
      }
      kw[((size_t)(i >> 2) * d.Nl + l) * 4u + (i & 3u)] = k;
    }
    const u64 used = cnt >= 64u ? ~0ull : (1ull << cnt) - 1ull;
    uint4 r2 = d.R2[l];
    r2.z = (r2.z & 0x7FFFu) | (cnt > HQ ? QDEEP : 0u) | ((u32)(used & 0xFFFFull) << 16);
    if (cnt > HQ) d.qused[l] = used;
    d.R2[l] = r2;
  }
}

__device__ static inline u64 dig(u64 w, u64 idx) { return mix64(w ^ (idx * 0xD1342543DE82EF95ull)); }
__device__ static inline void block_sum_add(u64 v, u64* out) {
  __shared__ u64 sm[BLOCK / 64];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int i = 0; i < BLOCK / 64; ++i) t += sm[i];
    atomicAdd((unsigned long long*)out, (unsigned long long)t);
  }
  __syncthreads();
}
// digest of a flat array whose physical word order IS the canonical order
__global__ void digest_flat(const u64* w, size_t n_words, u64* out) {
  u64 acc = 0;
  for (size_t i = blockIdx.x * (size_t)BLOCK + threadIdx.x; i < n_words; i += (size_t)gridDim.x * BLOCK) acc += dig(w[i], i);
  block_sum_add(acc, out);
}
// digest of a split array in its canonical (interleaved) word order: entry e = words 4e, 4e+1 (head), 4e+2, 4e+3 (tail)
__global__ void digest_split(const uint4* arr, size_t tail, size_t n_entries, u64* out) {
  u64 acc = 0;
  for (size_t e = blockIdx.x * (size_t)BLOCK + threadIdx.x; e < n_entries; e += (size_t)gridDim.x * BLOCK) {
    uint4 h = arr[e], t = arr[tail + e];
    acc += dig((u64)h.x | ((u64)h.y << 32), e * 4) + dig((u64)h.z | ((u64)h.w << 32), e * 4 + 1);
    acc += dig((u64)t.x | ((u64)t.y << 32), e * 4 + 2) + dig((u64)t.z | ((u64)t.w << 32), e * 4 + 3);
  }
  block_sum_add(acc, out);
}
// ... the share of the entries [from, to) of a split array when they are all zero (planes without memory: LazyPlanes)
__global__ void digest_split_zero(size_t from, size_t to, u64* out) {
  u64 acc = 0;
  for (size_t e = from + blockIdx.x * (size_t)BLOCK + threadIdx.x; e < to; e += (size_t)gridDim.x * BLOCK)
    acc += dig(0, e * 4) + dig(0, e * 4 + 1) + dig(0, e * 4 + 2) + dig(0, e * 4 + 3);
  block_sum_add(acc, out);
}
// running queries: tracker table, then the ack / response bitmaps (canonical order = physical order)
// ... then the filters (32-bit words) and the tag classes (bytes)
__global__ void digest_queries(const uint4* qtab, const u32* qbits, size_t n_bits_words, u32 N, u64* out) {
  u64 acc = 0;
  const size_t n0 = 2 * SIM_QT, n1 = n0 + n_bits_words, n2 = n1 + (size_t)SIM_QT * SIM_QF_WORDS, n3 = n2 + N;
  const u32* filt = reinterpret_cast<const u32*>(qtab + SIM_QT);
  const uint8_t* tags = reinterpret_cast<const uint8_t*>(qtab + SIM_QT + SIM_QT * (SIM_QF_WORDS / 4));
  for (size_t i = blockIdx.x * (size_t)BLOCK + threadIdx.x; i < n3; i += (size_t)gridDim.x * BLOCK) {
    if (i < n0) {
      uint4 t = qtab[i >> 1];
      u64 w = (i & 1) ? ((u64)t.z | ((u64)t.w << 32)) : ((u64)t.x | ((u64)t.y << 32));
      acc += dig(w, i);
    } else if (i < n1) {
      acc += dig((u64)qbits[i - n0], i);
    } else if (i < n2) {
      acc += dig((u64)filt[i - n1], i);
    } else {
      acc += dig((u64)tags[i - n2], i);
    }
  }
  block_sum_add(acc, out);
}
// one filter entry, by value (the host keeps the table and is its only writer)
struct QFiltEnt { uint4 w[SIM_QF_WORDS / 4]; };
__global__ void qfilt_set_kernel(uint4* dst, QFiltEnt e) {
  if (threadIdx.x < SIM_QF_WORDS / 4 && !blockIdx.x) dst[threadIdx.x] = e.w[threadIdx.x];
}
__global__ void query_count_kernel(const u32* bits, size_t words, u64* out /*[2]*/) {
  u64 a = 0, r = 0;
  for (size_t i = blockIdx.x * (size_t)BLOCK + threadIdx.x; i < words; i += (size_t)gridDim.x * BLOCK) {
    a += __popc(bits[i]);
    r += __popc(bits[words + i]);
  }
  block_sum_add(a, out);
  block_sum_add(r, out + 1);
}
// aux digest: slot map, then the liveness bitmap (bits past N masked)
__global__ void digest_aux(const u32* slot_of, const u32* upmap, u32 N, u64* out) {
  u64 acc = 0;
  size_t nw = ((size_t)N + 31) / 32;
  for (size_t i = blockIdx.x * (size_t)BLOCK + threadIdx.x; i < (size_t)N + nw; i += (size_t)gridDim.x * BLOCK) {
    if (i < N) {
      acc += dig((u64)slot_of[i], i);
    } else {
      size_t j = i - N;
      u32 w = upmap[j];
      if (j == N / 32 && (N & 31)) w &= (1u << (N & 31)) - 1u;
      acc += dig((u64)w, i);
    }
  }
  block_sum_add(acc, out);
}
__global__ void digest_rows_queue(Dev d, u64* out_rows, u64* out_queue) {
  u64 ar = 0, aq = 0;
  for (size_t l = blockIdx.x * (size_t)BLOCK + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * BLOCK) {
    u64 w[ROW_W];
    canon_row(d, l, w);
    for (int i = 0; i < ROW_W; ++i) ar += dig(w[i], l * ROW_W + i);
    u32 cnt = q_count(d, l, d.R2[l].z);
    for (u32 q = 0; q < SIM_Q; ++q) {
      uint4 e = canon_qrec(d, l, q, cnt);
      aq += dig((u64)e.x | ((u64)e.y << 32), (l * SIM_Q + q) * 2);
      aq += dig((u64)e.z | ((u64)e.w << 32), (l * SIM_Q + q) * 2 + 1);
    }
  }
  block_sum_add(ar, out_rows);
  block_sum_add(aq, out_queue);
}

__global__ void members_kernel(Dev d, const uint4* base, u32 obs_l, uint8_t* st, u64* lt) {
  for (size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x; s < d.N; s += (size_t)gridDim.x * blockDim.x) {
    u32 a = d.slot_of[s];
    uint4 e = a == NOSLOT ? base[s * 2] : d.view[(size_t)a * d.Nl + obs_l];
    bool known = e.w & SIM_VB_KNOWN;
    st[s] = known ? (uint8_t)SIM_VB_STATUS(e.w) : (uint8_t)SIM_STATUS_NONE;
    lt[s] = known ? E_LTIME(e) : 0;
  }
}
// up to SIM_CONV_MAX rumours in one pass (sim_convergence: one): out[0] = running nodes, out[1 + i] = those that have applied rumour i
struct ConvSet { u32 n; u32 kind[SIM_CONV_MAX], key[SIM_CONV_MAX]; u64 ltime[SIM_CONV_MAX]; };
__global__ void convergence_many_kernel(Dev d, const uint4* base, ConvSet cs, u64* out) {
  __shared__ u32 cnt[SIM_CONV_MAX + 1];
  for (u32 i = threadIdx.x; i <= SIM_CONV_MAX; i += BLOCK) cnt[i] = 0;
  __syncthreads();
  const size_t rounds = ((size_t)d.Nl + (size_t)gridDim.x * BLOCK - 1) / ((size_t)gridDim.x * BLOCK);
  for (size_t it = 0; it < rounds; ++it) {  // whole waves stay together: the ballots below need every lane
    size_t l = (it * gridDim.x + blockIdx.x) * (size_t)BLOCK + threadIdx.x;
    bool up = l < d.Nl && (d.R1[l].z & SIM_RF_UP);
    u64 m = __ballot(up);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[0], (u32)__popcll(m));
    for (u32 i = 0; i < cs.n; ++i) {
      bool hit = false;
      if (up) {
        u32 kind = cs.kind[i], key = cs.key[i];
        u64 ltime = cs.ltime[i];
        if (kind == SIM_K_JOIN || kind == SIM_K_LEAVE) {
          u32 a = d.slot_of[key];
          uint4 e = a == NOSLOT ? base[(size_t)key * 2] : d.view[(size_t)a * d.Nl + l];
          hit = view_applied(e, ltime);
        } else {
          const uint4* ring = kind == SIM_K_EVENT ? d.ering : d.qring;
          const u32 idx = (u32)(ltime % (kind == SIM_K_EVENT ? d.Bev : d.Bq));
          hit = bucket_holds(d, ring, kind == SIM_K_EVENT ? d.etail : d.qtail, idx, l, ring[(size_t)idx * d.Nl + l], key);
        }
      }
      u64 hm = __ballot(hit);
      if ((threadIdx.x & 63) == 0 && hm) atomicAdd(&cnt[1 + i], (u32)__popcll(hm));
    }
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i <= cs.n; i += BLOCK)
    if (cnt[i]) atomicAdd((unsigned long long*)(out + i), (unsigned long long)cnt[i]);
}
__global__ void stats_kernel(Dev d, u32 l, sim_stats* o) {
  if (threadIdx.x || blockIdx.x) return;
  sim_stats s;
  memset(&s, 0, sizeof s);
  uint4 r0 = d.R0[l], r1 = d.R1[l], r2 = d.R2[l], r3 = d.R3[l];
  s.members = r1.w; s.failed = r2.x; s.left = r2.y;
  s.health_score = r3.z;
  s.member_time = (u64)r0.x | ((u64)r0.y << 32);
  s.event_time = (u64)r0.z | ((u64)r0.w << 32);
  s.query_time = (u64)r1.x | ((u64)r1.y << 32);
  u32 cnt = q_count(d, l, r2.z);
  for (u32 q = 0; q < cnt; ++q) {
    uint4 kq = d.qkeys[(size_t)(q >> 2) * d.Nl + l];
    u32 k = (q & 3) == 0 ? kq.x : (q & 3) == 1 ? kq.y : (q & 3) == 2 ? kq.z : kq.w;
    u32 cls = k >> QK_CLS_SH;
    if (cls == 0) s.swim_queue++; else if (cls == 1) s.intent_queue++; else if (cls == 2) s.query_queue++; else s.event_queue++;
  }
  s.serf_state = SIM_RF_STATE(r1.z); s.up = r1.z & SIM_RF_UP; s.incarnation = r3.x;
  s.queue_overflow = r2.w;
  *o = s;
}
// cluster-wide load figures: out[0] up, [1..4] queue entries by class, [5] overflow, [6] records in flight,
// [7] failed, [8] left, [9] deepest queue (max)
// Two levels: every workgroup leaves its ten partial figures in part[blockIdx.x][10] (no atomics: 4096 workgroups adding to
// ten words cost 0.4 ms), cluster_stats_fold adds them up.
#define CSTAT_WG 1024
__global__ void cluster_stats_kernel(Dev d, const uint4* inbox, u64* part) {
  u64 a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  u32 mx = 0;
  for (size_t l = blockIdx.x * (size_t)BLOCK + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * BLOCK) {
    uint4 r1 = d.R1[l], r2 = d.R2[l];
    a[0] += (r1.z & SIM_RF_UP) ? 1u : 0u;
    u32 cnt = q_count(d, l, r2.z);
    mx = max(mx, cnt);
    for (u32 q = 0; q < cnt; ++q) {
      uint4 kq = d.qkeys[(size_t)(q >> 2) * d.Nl + l];
      u32 k = (q & 3) == 0 ? kq.x : (q & 3) == 1 ? kq.y : (q & 3) == 2 ? kq.z : kq.w;
      a[1 + (k >> QK_CLS_SH)] += 1;
    }
    a[5] += r2.w; a[7] += r2.x; a[8] += r2.y;
    if (inbox)
      for (u32 k = 0; k < d.fp; ++k)
        for (u32 p = 0; p < SIM_P; ++p) a[6] += SIM_META_KIND(pk_word(inbox[((size_t)k * d.Nl + l) * PK_U4 + 2], p)) != SIM_K_EMPTY;
  }
  __shared__ u64 sm[10][BLOCK / 64];
  for (int i = 0; i < 10; ++i) {
    const u64 v = i == 9 ? wave_max(mx) : wave_sum(a[i]);
    if ((threadIdx.x & 63) == 0) sm[i][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    u64 t = 0;
    for (int i = 0; i < BLOCK / 64; ++i) t = threadIdx.x == 9 ? max(t, sm[9][i]) : t + sm[threadIdx.x][i];
    part[(size_t)blockIdx.x * 10 + threadIdx.x] = t;
  }
}
__global__ void cluster_stats_fold(const u64* part, u32 nwg, u64* out) {  // one workgroup of 64 x 10 threads: figure = threadIdx.y
  const u32 i = threadIdx.y;
  u64 t = 0;
  for (u32 w = threadIdx.x; w < nwg; w += 64u) t = i == 9 ? max(t, part[(size_t)w * 10 + i]) : t + part[(size_t)w * 10 + i];
  t = i == 9 ? wave_max(t) : wave_sum(t);
  if (threadIdx.x == 0) out[i] = t;
}
// single-word / single-entry updates of device tables with the value passed by value (no host buffer to outlive)
__global__ void poke_u32(u32* p, u32 v) { if (!threadIdx.x && !blockIdx.x) *p = v; }
__global__ void poke_base(uint4* base, u32 x, uint4 e0, uint4 e1) { if (!threadIdx.x && !blockIdx.x) { base[(size_t)x * 2] = e0; base[(size_t)x * 2 + 1] = e1; } }
// ---- view-slot recycling scans (SIMSPEC §2.6; oracle recycle_scan) ----
// subjects that a running node still has a queued record or a suspicion timer about, or that a packet in flight mentions
// (packets in flight: sharded, the receive buffer `inbox`; local mode, inbox == null and the cells the senders kept —
// every cell a map word points at is delivered to somebody, so the set of subjects is the same)
__global__ void recycle_refd_kernel(Dev d, const uint4* inbox, u32 cur, uint8_t* refd, u32* first_up) {
  u32 lo = 0xFFFFFFFFu;
  for (size_t l = blockIdx.x * (size_t)BLOCK + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * BLOCK) {
    if (!inbox && !d.sharded && !d.rfan) {
      u32 jw = d.omap[cur][l];
      for (u32 k = 0; k < d.f; ++k) {
        u32 jb = (jw >> (8u * k)) & 0xFFu;  // first page << 2 | pages - 1
        bool again = jb == 0xFFu;
        for (u32 q = 0; q < k; ++q) again |= ((jw >> (8u * q)) & 0xFFu) == jb;
        if (again) continue;
        for (u32 pg = 0; pg <= (jb & 3u); ++pg) {
          const uint4* cellp = d.obox[cur] + ((size_t)((jb >> 2) + pg) * d.Nl + l) * PK_U4;
          uint4 ck = cellp[0], ch = cellp[2];
          for (u32 p = 0; p < SIM_P; ++p) {
            u32 key = pk_word(ck, p);
            if (member_kind(SIM_META_KIND(pk_word(ch, p))) && key < d.N) refd[key] = 1;
          }
        }
      }
    }
    if (d.rfan) {  // (r6) random fan-out: the senders' 64-byte cells, read where they lie — the map word sits in cell 0 (until r6: through the materialized inbox, 256 MB more)
      const u32 jw = d.obox[cur][(size_t)l * RF_CELL_U4 + 3u].x;
      for (u32 k = 0; k < d.f; ++k) {
        const u32 jb = (jw >> (8u * k)) & 0xFFu;  // first page << 2 | pages - 1
        bool again = jb == 0xFFu;
        for (u32 q = 0; q < k; ++q) again |= ((jw >> (8u * q)) & 0xFFu) == jb;
        if (again) continue;
        for (u32 pg = 0; pg <= (jb & 3u); ++pg) {
          const uint4* cellp = d.obox[cur] + ((size_t)((jb >> 2) + pg) * d.Nl + l) * RF_CELL_U4;
          const uint4 ck = cellp[0], ch = cellp[2];
          for (u32 p = 0; p < SIM_P; ++p) {
            const u32 key = pk_word(ck, p);
            if (member_kind(SIM_META_KIND(pk_word(ch, p))) && key < d.N) refd[key] = 1;
          }
        }
      }
    }
    if (inbox)
      for (u32 k = 0; k < d.fp; ++k)
        for (u32 p = 0; p < SIM_P; ++p) {
          const uint4* cellp = inbox + ((size_t)k * d.Nl + l) * PK_U4;
          u32 key = pk_word(cellp[0], p);
          if (member_kind(SIM_META_KIND(pk_word(cellp[2], p))) && key < d.N) refd[key] = 1;
        }
    uint4 r1 = d.R1[l];
    if (!(r1.z & SIM_RF_UP)) continue;
    lo = min(lo, (u32)l);
    u32 cnt = q_count(d, l, d.R2[l].z);
    for (u32 q = 0; q < cnt; ++q) {
      uint4 kq = d.qkeys[(size_t)(q >> 2) * d.Nl + l];
      u32 k = (q & 3) == 0 ? kq.x : (q & 3) == 1 ? kq.y : (q & 3) == 2 ? kq.z : kq.w;
      uint4 pay = d.qpay[(size_t)(k & QK_SLOT_MASK) * d.Nl + l];
      if (member_kind(SIM_META_KIND(pay.y)) && pay.x < d.N) refd[pay.x] = 1;
    }
    const uint16_t* sp = reinterpret_cast<const uint16_t*>(&d.R4[2 * l]);
    for (u32 j = 0; j < SIM_S; ++j)
      if (sp[j] && d.subject_of[sp[j] - 1] != NOSLOT) refd[d.subject_of[sp[j] - 1]] = 1;
  }
  if (lo != 0xFFFFFFFFu) atomicMin(first_up, lo);
}
// candidate c = blockIdx.y: does every running node hold the head the first running node holds?
// (r6: and, for the host, whether anything still mentions the candidate's subject — one word a candidate instead of the whole `refd` table)
__global__ void recycle_view_kernel(Dev d, const u32* cand_slots, const u32* first_up, uint4* out_ref, u32* out_bad, const uint8_t* refd, const u32* cand_subjects, u32* out_refd) {
  u32 c = blockIdx.y, a = cand_slots[c], l0 = *first_up;
  if (!blockIdx.x && !threadIdx.x) out_refd[c] = refd[cand_subjects[c]];
  if (l0 == 0xFFFFFFFFu) return;
  uint4 ref = d.view[(size_t)a * d.Nl + l0];
  ref.w &= 0x7FFu;  // the stamp of a settled entry is dead data
  if (!blockIdx.x && !threadIdx.x) out_ref[c] = ref;
  bool bad = false;
  for (size_t l = blockIdx.x * (size_t)BLOCK + threadIdx.x; l < d.Nl; l += (size_t)gridDim.x * BLOCK) {
    if (!(d.R1[l].z & SIM_RF_UP)) continue;
    uint4 e = d.view[(size_t)a * d.Nl + l];
    e.w &= 0x7FFu;
    bad |= ne4(e, ref);
  }
  if (bad) out_bad[c] = 1;
}
// Local mode, off the hot path: Dev::obox / omap (packets kept at their senders) <-> the canonical receiver-indexed
// inbox[k][node].  `p` = the parameters of the tick the packets were sent in; `valid` = 0 at tick 0 (nothing in flight).
__global__ void materialize_kernel(Dev d, TickP p, u32 cur, u32 valid, uint4* out) {
  size_t n = (size_t)d.fp * d.Nl;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    u32 kk = (u32)(i / d.Nl), l = (u32)(i - (size_t)kk * d.Nl), k = kk / d.PG, pg = kk - k * d.PG;
    uint4 a = make_uint4(0, 0, 0, 0), b = a, c = a;
    if (d.rfan) {  // random fan-out: the canonical form is the oracle's — packets in the SENDER's cells, [slot][sender]
      const u32 jb = valid ? (d.obox[cur][(size_t)l * RF_CELL_U4 + 3u].x >> (8u * k)) & 0xFFu : 0xFFu;  // the map word sits in cell 0
      if (jb != 0xFFu && pg <= (jb & 3u)) {
        const uint4* cp = d.obox[cur] + ((size_t)((jb >> 2) + pg) * d.Nl + l) * RF_CELL_U4;
        a = cp[0]; b = cp[1]; c = cp[2];
      }
    } else if (valid && k < p.feff) {
      u32 h = l / p.M, t = l - h * p.M, g, ll;
      fan_source_g(p, PICK4(p.off, k), PICK4(p.rot, k), PICK4(p.rho, k), h, t, k, g, ll);
      u32 s = g * p.M + ll;
      u32 jb = (d.omap[cur][s] >> (8u * k)) & 0xFFu;  // first page << 2 | pages - 1
      if (jb != 0xFFu && pg <= (jb & 3u)) {
        const uint4* cp = d.obox[cur] + ((size_t)((jb >> 2) + pg) * d.Nl + s) * PK_U4;
        a = cp[0]; b = cp[1]; c = cp[2];
      }
    }
    out[i * PK_U4] = a; out[i * PK_U4 + 1] = b; out[i * PK_U4 + 2] = c;
  }
}
__global__ void unmaterialize_kernel(Dev d, TickP p, u32 cur, u32 valid, const uint4* in) {
  for (size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x; s < d.Nl; s += (size_t)gridDim.x * blockDim.x) {
    if (d.rfan) {  // random fan-out: the image is sender-indexed already; every slot gets its own pages k * PG ..., the map word goes into cell 0
      u32 jw = 0xFFFFFFFFu;
      for (u32 k = 0; valid && k < d.f; ++k) {
        u32 np = 0;
        for (u32 pg = 0; pg < d.PG; ++pg) {
          const uint4* cp = in + ((size_t)(k * d.PG + pg) * d.Nl + s) * PK_U4;
          uint4 a = cp[0], b = cp[1], c = cp[2];
          if (((c.x | c.y | c.z | c.w) & 0xF0u) == 0) break;
          uint4* op = d.obox[cur] + ((size_t)(k * d.PG + pg) * d.Nl + s) * RF_CELL_U4;
          op[0] = a; op[1] = b; op[2] = c;
          np = pg + 1;
        }
        if (np) jw = (jw & ~(0xFFu << (8u * k))) | ((((k * d.PG) << 2) | (np - 1u)) << (8u * k));
      }
      d.obox[cur][(size_t)s * RF_CELL_U4 + 3u] = make_uint4(jw, 0u, 0u, 0u);
      continue;
    }
    u32 jw = 0xFFFFFFFFu;
    if (valid) {
      u32 g = (u32)s / p.M, ll = (u32)s - g * p.M;
      for (u32 k = 0; k < p.feff; ++k) {  // every slot gets its own pages k * PG ...: an image does not say which packets were the same
        u32 h, t, np = 0;
        fan_target_g(p, g, ll, k, h, t);
        for (u32 pg = 0; pg < d.PG; ++pg) {
          const uint4* cp = in + ((size_t)(k * d.PG + pg) * d.Nl + (size_t)h * p.M + t) * PK_U4;
          uint4 a = cp[0], b = cp[1], c = cp[2];
          if (((c.x | c.y | c.z | c.w) & 0xF0u) == 0) break;  // no record in it: pages fill up in order
          uint4* op = d.obox[cur] + ((size_t)(k * d.PG + pg) * d.Nl + s) * PK_U4;
          op[0] = a; op[1] = b; op[2] = c;
          np = pg + 1;
        }
        if (np) jw = (jw & ~(0xFFu << (8u * k))) | ((((k * d.PG) << 2) | (np - 1u)) << (8u * k));
      }
    }
    d.omap[cur][s] = jw;
  }
}
__global__ void set_flag_bits(uint4* R1, u32 l, u32 bits) {
  if (threadIdx.x == 0 && blockIdx.x == 0) R1[l].z |= bits;
}
