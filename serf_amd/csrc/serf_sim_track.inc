// serf_sim_track.inc — part of the translation unit serf_sim.hip (included from there, last; not a header of its own).
// Device-resident trackers (include/serf_sim_track.h): two kernels behind a tick's last launch, the host's bookkeeping, the entry points.
//
// Per tick with at least one tracker inside its window:
//   track_count_kernel    a node per lane (four at a time); counts, per tracker, the running nodes whose predicate holds: ballots into LDS
//                         counters, one column of partial counts per workgroup — integers throughout, no atomics on global memory
//   track_resolve_kernel  one wave per tracker; adds the partial counts up, compares count and running nodes with the thresholds, writes
//                         latches / peak / last into the result table on the device, retires
// Their order is the stream's.  The host knows every window, so it builds a tick's list without reading anything back; the list goes to
// the device only when it CHANGES (a window opens or closes, add / remove, a retirement the host has learnt of), through pinned staging
// buffers, without a blocking copy.  Retirements come back through a word per tracker of pinned memory the resolve kernel sets: the
// host looks at them in sim_step_end, without waiting — until it has seen one, the count kernel skips the retired tracker itself.  A handle without a registered tracker never gets here (sim_step_end tests one pointer).
#include "../../include/serf_sim_track.h"

static_assert(sizeof(sim_tracker) == 32 && sizeof(sim_track_result) == 56, "layout of include/serf_sim_track.h");

// one entry of the tick's list: the tracker as the kernel needs it.  pkey names the 16-byte plane it reads — the list is sorted by it, so
// the trackers of one plane are neighbours and a wave loads the plane's head once for all of them
struct TrkItem {
  u32 pkey;     // TRK_PK_VIEW | subject,  TRK_PK_EV | bucket,  TRK_PK_Q | bucket
  u32 id;       // entry of the result table
  u32 a;        // EVENT / QUERY: the key;  MEMBER: low half of the predicate's table (below)
  u32 b;        // MEMBER: min_inc;  JOIN / LEAVE: low half of the Lamport time
  u32 c;        // MEMBER: high half of the table;  JOIN / LEAVE: high half of the Lamport time
  u32 member;   // 1: MEMBER predicate, 0: RUMOUR
  u32 nxt;      // list position of the first entry of the NEXT plane (n: none): its head is requested while this plane's trackers are tested
  u32 pad;
};
// MEMBER: the predicate over (known, MemberStatus, swim state) is a table of 64 bits indexed by the low six bits of sim_view.bits —
// [0] known, [3:1] status, [5:4] swim — made by the host from the two masks: one shift and one test per node instead of three fields
static_assert(sizeof(TrkItem) == 32, "TrkItem");
#define TRK_PK_VIEW 0x00000000u
#define TRK_PK_EV 0x80000000u
#define TRK_PK_Q 0xC0000000u
#define TRK_PK_NONE 0x7FFFFFFFu  // (node ids have 24 bits: no subject's key)
#define TRK_PK_SKIP 0x7FFFFFFEu  // a tracker that has retired and is still in the list
#define TRK_RING 4       // pinned staging buffers of the list
#define TRK_GRID 1024u   // workgroups of the count kernel at most: each stages the list once and walks its share of the nodes
#define TRK_NPL 4        // nodes per lane and pass: four independent plane loads in flight per lane (and four more one plane ahead)

struct TrkDevP {
  const TrkItem* items;     // [n] the tick's list
  const u32* end_tick;      // [SIM_TRACK_MAX] by id: the tick after the last one of the window (0: none)
  sim_track_result* res;    // [SIM_TRACK_MAX] by id
  u32* part;                // [n + 1][G] partial counts by list position and workgroup of the count kernel (row n: running nodes): every
                            //   workgroup writes its column, the resolve kernel adds the rows up — no atomics on global memory, nothing to zero
  u32* h_ret;               // [SIM_TRACK_MAX] by id, pinned host memory: set when the tracker retires — the host drops retired trackers
                            //   from its lists without waiting for anything
  u32 n;
  u32 G;                    // workgroups of the count kernel
  u32 now;                  // sim_tick after the tick being evaluated
};

__device__ static inline uint4 trk_head(const Dev& d, const uint4* __restrict__ base, u32 pkey, size_t l) {
  if (pkey < TRK_PK_EV) {  // the subject's view slot is looked up now: slots are handed out and recycled while trackers live
    const u32 a = d.slot_of[pkey];
    return a == NOSLOT ? base[(size_t)pkey * 2] : d.view[(size_t)a * d.Nl + l];
  }
  const uint4* ring = pkey >= TRK_PK_Q ? d.qring : d.ering;
  return ring[(size_t)(pkey & 0x3FFFFFFFu) * d.Nl + l];
}

__global__ __launch_bounds__(BLOCK) void track_count_kernel(Dev d, const uint4* __restrict__ base, TrkDevP p) {
  __shared__ u32 lcnt[SIM_TRACK_MAX];  // the counters: 4 KiB
  __shared__ u32 lup;
  // the list, staged once per workgroup (a wave reads an entry at one address: a broadcast): 18 KiB
  __shared__ u32 s_pkey[SIM_TRACK_MAX], s_a[SIM_TRACK_MAX], s_b[SIM_TRACK_MAX], s_c[SIM_TRACK_MAX];
  __shared__ unsigned short s_nxt[SIM_TRACK_MAX];  // | 0x8000: MEMBER
  for (u32 i = threadIdx.x; i < p.n; i += BLOCK) {
    const TrkItem t = p.items[i];
    lcnt[i] = 0;
    s_pkey[i] = p.res[t.id].state == 2 ? TRK_PK_SKIP : t.pkey;  // retired by `all` before the host has learnt of it
    s_a[i] = t.a;
    s_b[i] = t.b;
    s_c[i] = t.c;
    s_nxt[i] = (unsigned short)(t.nxt | (t.member ? 0x8000u : 0u));  // (nxt <= SIM_TRACK_MAX)
  }
  if (!threadIdx.x) lup = 0;
  __syncthreads();
  const bool lane0 = (threadIdx.x & 63) == 0;
  const size_t per_pass = (size_t)gridDim.x * BLOCK * TRK_NPL;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together: the ballots below need every lane
    size_t l[TRK_NPL];
    bool up[TRK_NPL];
    u32 nup = 0;
#pragma unroll
    for (int k = 0; k < TRK_NPL; ++k) {
      l[k] = it * per_pass + ((size_t)blockIdx.x * TRK_NPL + k) * BLOCK + threadIdx.x;
      up[k] = l[k] < d.Nl && (d.R1[l[k]].z & SIM_RF_UP);
      nup += (u32)__popcll(__ballot(up[k]));
    }
    if (!nup) continue;  // (wave-uniform) nobody of these nodes is running
    if (lane0) atomicAdd(&lup, nup);
    u32 cur = TRK_PK_NONE, pfk = TRK_PK_NONE;
    uint4 e[TRK_NPL], pfe[TRK_NPL];
#pragma unroll
    for (int k = 0; k < TRK_NPL; ++k) e[k] = pfe[k] = make_uint4(0, 0, 0, 0);
    for (u32 i = 0; i < p.n; ++i) {
      // an entry is the same for every lane: through the scalar registers, so that what depends on it alone branches for the wave
      const u32 pkey = __builtin_amdgcn_readfirstlane(s_pkey[i]);
      if (pkey == TRK_PK_SKIP) continue;
      const u32 nx = __builtin_amdgcn_readfirstlane((u32)s_nxt[i]);
      if (pkey != cur) {  // the plane's head: 16 bytes a node, node index fastest — asked for one plane ahead
        cur = pkey;
        if (pfk == pkey) {
#pragma unroll
          for (int k = 0; k < TRK_NPL; ++k) e[k] = pfe[k];
        } else {
#pragma unroll
          for (int k = 0; k < TRK_NPL; ++k)
            if (up[k]) e[k] = trk_head(d, base, pkey, l[k]);
        }
        const u32 j = nx & 0x7FFFu;
        pfk = j < p.n ? __builtin_amdgcn_readfirstlane(s_pkey[j]) : TRK_PK_NONE;
        if (pfk == TRK_PK_SKIP) pfk = TRK_PK_NONE;
        if (pfk != TRK_PK_NONE) {
#pragma unroll
          for (int k = 0; k < TRK_NPL; ++k)
            if (up[k]) pfe[k] = trk_head(d, base, pfk, l[k]);
        }
      }
      const u32 ta = __builtin_amdgcn_readfirstlane(s_a[i]), tb = __builtin_amdgcn_readfirstlane(s_b[i]), tc = __builtin_amdgcn_readfirstlane(s_c[i]);
      u32 hits = 0;
#pragma unroll
      for (int k = 0; k < TRK_NPL; ++k) {
        const uint4 ek = e[k];
        bool hit = false;
        if (pkey < TRK_PK_EV) {
          if (nx & 0x8000u) {  // MEMBER
            const u64 table = (u64)ta | ((u64)tc << 32);
            hit = up[k] && ((table >> (ek.w & 63u)) & 1u) && ek.z >= tb;
          } else {
            hit = up[k] && view_applied(ek, (u64)tb | ((u64)tc << 32));
          }
        } else {
          // bucket_holds (serf_sim_observe.inc) written out, without its test for key 0 (track_check refuses that key): this kernel
          // uses every SGPR there is, and with the call — in any of the forms tried — the compiler spills two to six of them
          hit = up[k] && ((ek.z == ta) | (ek.w == ta));
          if (up[k] && !hit && ek.w) {  // the tail plane only when the head is full and does not hold the key
            const bool q = pkey >= TRK_PK_Q;
            const uint4* ring = q ? d.qring : d.ering;
            const size_t tl = q ? d.qtail : d.etail;
            const u32 idx = pkey & 0x3FFFFFFFu;
            const uint4 b1 = ring[(size_t)idx * d.Nl + l[k] + tl];
            hit = (b1.x == ta) | (b1.y == ta) | (b1.z == ta) | (b1.w == ta);
            if (!hit && b1.w) hit = ovf_has(d, ring, tl, (u32)l[k], idx, ta);  // a full bucket: its overflow rows
          }
        }
        hits += (u32)__popcll(__ballot(hit));
      }
      if (lane0 && hits) atomicAdd(&lcnt[i], hits);
    }
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < p.n; i += BLOCK) p.part[(size_t)i * p.G + blockIdx.x] = lcnt[i];
  if (!threadIdx.x) p.part[(size_t)p.n * p.G + blockIdx.x] = lup;
}

// one wave per tracker of the list: adds up its row of partial counts (and the row of the running nodes), then one lane decides
__global__ __launch_bounds__(BLOCK) void track_resolve_kernel(TrkDevP p) {
  const u32 i = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= p.n) return;  // (whole waves)
  const u64 c = fold_row(p.part + (size_t)i * p.G, p.G, FOLD_SUM), up = fold_row(p.part + (size_t)p.n * p.G, p.G, FOLD_SUM);
  if (lane) return;
  const u32 id = p.items[i].id;
  sim_track_result r = p.res[id];
  if (r.state == 2) return;
  r.evaluated++;
  r.last = c;
  r.last_up = up;
  if (c > r.peak) r.peak = c;
  if (up) {
    if (r.first == SIM_TRACK_NEVER && c >= 1) r.first = p.now;
    if (r.half == SIM_TRACK_NEVER && 2 * c >= up) r.half = p.now;
    if (r.p90 == SIM_TRACK_NEVER && 10 * c >= 9 * up) r.p90 = p.now;
    if (r.p99 == SIM_TRACK_NEVER && 100 * c >= 99 * up) r.p99 = p.now;
    if (r.all == SIM_TRACK_NEVER && c == up) r.all = p.now;
  }
  r.state = (r.all != SIM_TRACK_NEVER || p.end_tick[id] == p.now) ? 2u : 1u;
  p.res[id] = r;
  if (r.state == 2) p.h_ret[id] = 1;
}

// ---- host ----
struct TrackState {
  struct Ent {
    bool used = false, retired = false;  // retired: the host KNOWS it (window over, or state 2 read back)
    TrkItem item;
    u64 start = 0, end = 0;              // evaluated after ticks start .. end - 1 (end 0: no age)
  };
  Ent ent[SIM_TRACK_MAX];
  u32 n_reg = 0;
  // device
  TrkItem* d_items = nullptr;
  u32* d_end = nullptr;
  sim_track_result* d_res = nullptr;
  u32* d_part = nullptr;
  u32* h_ret = nullptr;  // pinned [SIM_TRACK_MAX]; written by track_resolve_kernel, read by sim_step_end without waiting
  // the list in use and its staging
  TrkItem* stage[TRK_RING] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t stage_ev[TRK_RING] = {nullptr, nullptr, nullptr, nullptr};
  bool stage_busy[TRK_RING] = {false, false, false, false};
  u32 stage_i = 0;
  u32 n_list = 0;        // entries of the list on the device
  bool dirty = true;     // the list has to be rebuilt before the next evaluation
  u64 next_change = 0;   // the first tick at which a window opens or closes
  sim_track_result* h_res = nullptr;  // pinned [SIM_TRACK_MAX]: what sim_track_read / the compaction read back
};

static void track_destroy(sim_handle* h) {
  TrackState* s = h->trk;
  if (!s) return;
  for (int i = 0; i < TRK_RING; ++i) {
    if (s->stage[i]) (void)hipHostFree(s->stage[i]);
    if (s->stage_ev[i]) (void)hipEventDestroy(s->stage_ev[i]);
  }
  if (s->h_res) (void)hipHostFree(s->h_res);
  if (s->h_ret) (void)hipHostFree(s->h_ret);
  if (s->d_items) (void)hipFree(s->d_items);
  if (s->d_end) (void)hipFree(s->d_end);
  if (s->d_res) (void)hipFree(s->d_res);
  if (s->d_part) (void)hipFree(s->d_part);
  delete s;
  h->trk = nullptr;
}
// the first sim_track_add of a handle: the tables (a handle that never tracks allocates nothing)
static int track_init(sim_handle* h) {
  if (h->trk) return SIM_OK;
  TrackState* s = new TrackState();
  h->trk = s;
  bool ok = hipMalloc((void**)&s->d_items, SIM_TRACK_MAX * sizeof(TrkItem)) == hipSuccess &&
            hipMalloc((void**)&s->d_end, SIM_TRACK_MAX * 4) == hipSuccess &&
            hipMalloc((void**)&s->d_res, SIM_TRACK_MAX * sizeof(sim_track_result)) == hipSuccess &&
            hipMalloc((void**)&s->d_part, (size_t)(SIM_TRACK_MAX + 1) * TRK_GRID * 4) == hipSuccess &&
            hipHostMalloc((void**)&s->h_ret, SIM_TRACK_MAX * 4, hipHostMallocDefault) == hipSuccess &&
            hipHostMalloc((void**)&s->h_res, SIM_TRACK_MAX * sizeof(sim_track_result), hipHostMallocDefault) == hipSuccess;
  for (int i = 0; ok && i < TRK_RING; ++i)
    ok = hipHostMalloc((void**)&s->stage[i], SIM_TRACK_MAX * sizeof(TrkItem), hipHostMallocDefault) == hipSuccess &&
         hipEventCreateWithFlags(&s->stage_ev[i], hipEventDisableTiming) == hipSuccess;
  if (ok) memset(s->h_ret, 0, SIM_TRACK_MAX * 4);
  if (ok) ok = hipMemsetAsync(s->d_end, 0, SIM_TRACK_MAX * 4, h->stream) == hipSuccess &&
               hipMemsetAsync(s->d_res, 0, SIM_TRACK_MAX * sizeof(sim_track_result), h->stream) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); track_destroy(h); return SIM_ENOMEM; }
  return SIM_OK;
}
// the list of tick t (the tick that just ended): every tracker inside its window that the host does not know to be retired, sorted by
// plane; enqueued behind whatever still reads the list before it
static int track_rebuild(sim_handle* h, u64 t) {
  TrackState* s = h->trk;
  std::vector<TrkItem> v;
  u64 nc = ~0ull;
  for (u32 id = 0; id < SIM_TRACK_MAX; ++id) {
    TrackState::Ent& e = s->ent[id];
    if (!e.used || e.retired) continue;
    if (e.end && t >= e.end) { e.retired = true; continue; }  // its last tick has been evaluated: the resolve kernel retired it
    if (e.start > t) { nc = std::min(nc, e.start); continue; }
    if (e.end) nc = std::min(nc, e.end);
    v.push_back(e.item);
  }
  std::sort(v.begin(), v.end(), [](const TrkItem& a, const TrkItem& b) { return a.pkey != b.pkey ? a.pkey < b.pkey : a.id < b.id; });
  for (size_t i = v.size(), nx = v.size(); i-- > 0;) {  // where the next plane's trackers begin
    if (i + 1 < v.size() && v[i + 1].pkey != v[i].pkey) nx = i + 1;
    v[i].nxt = (u32)nx;
  }
  s->next_change = nc;
  s->dirty = false;
  s->n_list = (u32)v.size();
  if (v.empty()) return SIM_OK;
  const u32 b = s->stage_i++ % TRK_RING;
  if (s->stage_busy[b]) HCHECK(hipEventSynchronize(s->stage_ev[b]));  // (the copy of four list changes ago: long done)
  memcpy(s->stage[b], v.data(), v.size() * sizeof(TrkItem));
  HCHECK(hipMemcpyAsync(s->d_items, s->stage[b], v.size() * sizeof(TrkItem), hipMemcpyHostToDevice, h->stream));
  HCHECK(hipEventRecord(s->stage_ev[b], h->stream));
  s->stage_busy[b] = true;
  return SIM_OK;
}
// sim_step_end: tick h->tick - 1 has been enqueued; its evaluation follows it on the stream
static int track_step_end(sim_handle* h) {
  TrackState* s = h->trk;
  if (!s->n_reg) return SIM_OK;
  const u64 t = h->tick - 1;
  // retirements the resolve kernel has reported so far (pinned words, set once while an id is in use: a value that is a few ticks old
  // is merely late): those trackers leave the list
  for (u32 id = 0; id < SIM_TRACK_MAX; ++id) {
    TrackState::Ent& e = s->ent[id];
    if (((volatile u32*)s->h_ret)[id] && e.used && !e.retired) { e.retired = true; s->dirty = true; }
  }
  if (s->dirty || t >= s->next_change) { if (int rc = track_rebuild(h, t)) return rc; }
  if (!s->n_list) return SIM_OK;
  TrkDevP p;
  p.items = s->d_items; p.end_tick = s->d_end; p.res = s->d_res; p.part = s->d_part; p.h_ret = s->h_ret;
  p.n = s->n_list; p.now = (u32)h->tick;
  p.G = (u32)std::min<size_t>(((size_t)h->d.Nl + BLOCK * TRK_NPL - 1) / (BLOCK * TRK_NPL), TRK_GRID);
  track_count_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d, h->d_base, p);
  track_resolve_kernel<<<(p.n + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
  HCHECK(hipGetLastError());
  return SIM_OK;
}
// the stream is idle: the result table comes to the host; trackers that retired by `all` leave the list
static int track_fetch(sim_handle* h) {
  TrackState* s = h->trk;
  HCHECK(hipMemcpyAsync(s->h_res, s->d_res, SIM_TRACK_MAX * sizeof(sim_track_result), hipMemcpyDeviceToHost, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  for (u32 id = 0; id < SIM_TRACK_MAX; ++id) {
    TrackState::Ent& e = s->ent[id];
    if (e.used && !e.retired && s->h_res[id].state == 2) { e.retired = true; s->dirty = true; }
  }
  return SIM_OK;
}

static int track_check(const sim_handle* h, const sim_tracker& t, TrkItem* it) {
  const Dev& d = h->d;
  memset(it, 0, sizeof *it);
  if (t.kind == SIM_TRK_MEMBER) {
    const u32 sm = t.b & 0xFFu, wm = t.b >> 8;
    if (t.a >= d.N || t.ltime || !t.b || sm >= (1u << (SIM_STATUS_FAILED + 1)) || wm >= (1u << (SIM_SWIM_LEFT + 1))) return SIM_EINVAL;
    u64 table = 0;  // over the low six bits of sim_view.bits
    for (u32 code = 0; code < 64; ++code) {
      const bool known = code & SIM_VB_KNOWN;
      const u32 st = known ? SIM_VB_STATUS(code) : (u32)SIM_STATUS_NONE;
      if (((sm >> st) & 1u) || (known && ((wm >> SIM_VB_SWIM(code)) & 1u))) table |= 1ull << code;
    }
    it->pkey = TRK_PK_VIEW | t.a; it->a = (u32)table; it->c = (u32)(table >> 32); it->b = t.min_inc; it->member = 1;
  } else if (t.kind == SIM_TRK_RUMOUR) {
    if (t.min_inc) return SIM_EINVAL;
    if (t.a == SIM_K_JOIN || t.a == SIM_K_LEAVE) {
      if (t.b >= d.N) return SIM_EINVAL;
      it->pkey = TRK_PK_VIEW | t.b; it->b = (u32)t.ltime; it->c = (u32)(t.ltime >> 32);
    } else if (t.a == SIM_K_EVENT || t.a == SIM_K_QUERY) {
      if (!t.b) return SIM_EINVAL;
      const bool q = t.a == SIM_K_QUERY;
      it->pkey = (q ? TRK_PK_Q : TRK_PK_EV) | (u32)(t.ltime % (q ? d.Bq : d.Bev));
      it->a = t.b;
    } else return SIM_EINVAL;
  } else return SIM_EINVAL;
  return SIM_OK;
}

extern "C" {

uint32_t sim_track_version(void) { return SIM_TRACK_VERSION; }

int sim_track_add(sim_handle* h, const sim_tracker* t, uint32_t n, uint32_t* ids_out) {
  if (int rc = observer_usable(h)) return rc;
  if (!t || !ids_out || !n) return SIM_EINVAL;
  std::vector<TrkItem> items(std::min<u32>(n, SIM_TRACK_MAX + 1));
  for (u32 i = 0; i < n && i <= SIM_TRACK_MAX; ++i)
    if (int rc = track_check(h, t[i], &items[i])) return rc;
  if (n > SIM_TRACK_MAX || (h->trk ? h->trk->n_reg : 0u) + n > SIM_TRACK_MAX) return SIM_ERANGE;
  if (int rc = track_init(h)) return rc;
  // a ring plane is made resident before a kernel may read it (the route sim_convergence takes)
  for (u32 i = 0; i < n; ++i)
    if (t[i].kind == SIM_TRK_RUMOUR)
      if (int rc = conv_plane(h, t[i].a, t[i].ltime)) return rc;
  TrackState* s = h->trk;
  // the entries' rows of the device tables are written with the stream idle: whatever evaluated a former owner of an id is done
  HCHECK(hipStreamSynchronize(h->stream));
  u32 id = 0;
  for (u32 i = 0; i < n; ++i) {
    while (s->ent[id].used) ++id;  // (n_reg + n <= SIM_TRACK_MAX: there is one)
    TrackState::Ent& e = s->ent[id];
    e.used = true; e.retired = false;
    e.item = items[i];
    e.item.id = id;
    e.start = std::max<u64>(t[i].start_tick, h->tick);
    e.end = t[i].max_age ? e.start + t[i].max_age : 0;
    if (e.end > 0xFFFFFFFFull) e.end = 0;  // (a window that ends beyond what a 32-bit tick can name never ends)
    sim_track_result r;
    memset(&r, 0, sizeof r);
    r.first = r.half = r.p90 = r.p99 = r.all = SIM_TRACK_NEVER;
    const u32 end32 = (u32)e.end;
    HCHECK(hipMemcpy(s->d_res + id, &r, sizeof r, hipMemcpyHostToDevice));
    HCHECK(hipMemcpy(s->d_end + id, &end32, 4, hipMemcpyHostToDevice));
    s->h_ret[id] = 0;  // (the stream is idle: nobody else writes this word now)
    ids_out[i] = id;
    s->n_reg++;
  }
  s->dirty = true;
  return SIM_OK;
}

static int track_ids_ok(const sim_handle* h, const uint32_t* ids, uint32_t n, bool distinct) {
  if (!ids || !n || !h->trk) return SIM_EINVAL;
  for (u32 i = 0; i < n; ++i) {
    if (ids[i] >= SIM_TRACK_MAX || !h->trk->ent[ids[i]].used) return SIM_EINVAL;
    if (distinct)
      for (u32 j = 0; j < i; ++j)
        if (ids[j] == ids[i]) return SIM_EINVAL;
  }
  return SIM_OK;
}

int sim_track_remove(sim_handle* h, const uint32_t* ids, uint32_t n) {
  if (int rc = observer_usable(h)) return rc;
  if (n > SIM_TRACK_MAX) return SIM_EINVAL;
  if (int rc = track_ids_ok(h, ids, n, true)) return rc;
  TrackState* s = h->trk;
  for (u32 i = 0; i < n; ++i) { s->ent[ids[i]].used = false; s->n_reg--; }
  s->dirty = true;  // (evaluations already enqueued still name the entries; sim_track_add waits for them before it reuses one)
  return SIM_OK;
}

int sim_track_read(sim_handle* h, const uint32_t* ids, uint32_t n, sim_track_result* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out) return SIM_EINVAL;
  if (int rc = track_ids_ok(h, ids, n, false)) return rc;
  if (int rc = track_fetch(h)) return rc;
  for (u32 i = 0; i < n; ++i) out[i] = h->trk->h_res[ids[i]];
  return SIM_OK;
}

int sim_track_active(sim_handle* h, uint32_t* registered, uint32_t* active) {
  if (int rc = observer_usable(h)) return rc;
  if (!registered || !active) return SIM_EINVAL;
  *registered = *active = 0;
  TrackState* s = h->trk;
  if (!s || !s->n_reg) return SIM_OK;
  if (int rc = track_fetch(h)) return rc;
  for (u32 id = 0; id < SIM_TRACK_MAX; ++id)
    if (s->ent[id].used) { ++*registered; *active += s->h_res[id].state != 2; }
  return SIM_OK;
}

}  // extern "C"
