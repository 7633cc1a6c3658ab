// serf_sim_tree.inc — part of the translation unit serf_sim.hip (included from there, after the traffic meter; not a header of its own).
// Rumour tree (include/serf_sim_tree.h): four kernels behind every sampled tick's last launch, the kernels of the reads, the host's
// bookkeeping, the entry points.
//
// Per sampled tick, in stream order:
//   tree_latch_kernel  a node per lane, grid-stride, TREE_GRID workgroups at most, whole waves kept together.  The entries — uploaded at sim_tree_start as the ledger's table, index included — are staged once
//                      per workgroup in LDS (lds_stage).  Per (node, entry): one coalesced 4-byte read of the arrival plane; the shared predicate
//                      (rumour_held) only for a running node that has no arrival yet.  Where a node latches, its candidate — which lies in
//                      the parent plane itself, scratch until now, valid when the node's bit of cmask[l] is set and the host says the
//                      previous sample's stamp is now - 1 — is judged by its own arrival (a != 0 && a < now: a parent latching in this
//                      launch reads as 0 or as now, and neither counts) and parent / hop are frozen.  have[l], a 64-bit mask of the
//                      entries the node has an arrival for, is written whole, one coalesced 8-byte store
//   tree_carry_kernel  the sender side (sent_packets, serf_sim_observe.inc): all three uint4 of every page of every DISTINCT packet the
//                      node sent; a record's identity is looked up in the LDS index (ledger_find).  One 64-bit carry mask per (slot, node) — a plane per slot —, copied to the slots that map to the
//                      same packet; `copies` through LDS adds, weighted by those slots (the ledger's word 6, counted the ledger's way)
//   tree_cand_kernel   the receiver side (recv_packets; flight_fill puts the graph of the sampled tick in front of the stream under
//                      kRandomNodes).  One 8-byte gather per packet, and-ed with ~have[l]; per set bit a minimum into the
//                      node's own candidate — a lane owns its node: no race —; cmask[l] says which entries got one.  `fresh` through LDS adds
//   tree_fold_kernel   one wave per word of the sample (fold_row).  `reached` and `orphans so far` are the previous sample's words plus
//                      this sample's new ones: arrivals are written by samples only and the samples lie one behind the other
// The count kernels write their workgroup's column of ONE partial matrix [1 + TREE_ROWS n][G] as 64-bit words — no atomics on global
// memory, nothing to zero, every figure an integer, the result does not depend on order.  The planes are [n][Nl] uint32_t each, the
// masks [Nl] / [4][Nl] uint64_t: every access of a wave to its own nodes is one contiguous run.
// The reads (each behind a wait for the stream — observer_settle —, on scratch of its own, the tree untouched):
//   tree_children_kernel   children[parent[l]] += 1 on zeroed scratch: integer atomicAdd, the result does not depend on order
//   tree_links_kernel      a slice of the three planes and the scratch transposed into 16-byte records
//   tree_stat_kernel / tree_stat_fold   one entry's summary in one pass, its columns folded
//   tree_path_kernel       one lane chases parent[] from the node to its orphan, hop + 1 ids
//   tree_top_kernel / tree_top_fold     the ranking in two levels (rank_candidates / rank_merge) by (children << 32) | (0xFFFFFFFF - id)
// A handle without a started tree never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_tree.h"

static_assert(sizeof(sim_tree_entry) == 16 && sizeof(sim_tree_entry) == sizeof(sim_ledger_entry) && offsetof(sim_tree_entry, ltime) == offsetof(sim_ledger_entry, val) &&
              sizeof(sim_tree_link) == 16 && sizeof(sim_tree_rank) == 24 && SIM_TREE_MAX == SIM_SPREAD_MAX && SIM_TREE_MAX == SIM_LEDGER_MAX &&
              SIM_TREE_MAX == 64u && SIM_TREE_HEADER_WORDS == 8u && SIM_TREE_ENTRY_WORDS == 8u && SIM_TREE_BINS == 32u && SIM_TREE_SUMMARY_WORDS == 72u,
              "layout of include/serf_sim_tree.h; an entry is the spread map's and goes into the ledger's table; the masks have 64 bits");
static_assert(SIM_TREE_TOP_MAX <= BLOCK, "a workgroup has top_k candidates at most among its BLOCK nodes");
static_assert(SIM_MAX_FANOUT == 4u, "a carry plane per fan-out slot");

#define TREE_GRID 1024u      // workgroups of the per-tick kernels and of the summary's pass at most
#define TREE_ROWS 4u         // rows of the partial matrix an entry: new, new orphans (latch), copies (carry), fresh (cand)
#define TREE_RANK_WORDS 3u   // a sim_tree_rank as 64-bit words
// words of the header, of an entry and of an entry's summary (include/serf_sim_tree.h)
enum { TH_TICK = 0, TH_UP = 1, TH_N = 2, TH_NEW = 3, TH_ORPHANS = 4, TH_COPIES = 5, TH_FRESH = 6 };
enum { TE_ID = 0, TE_VAL = 1, TE_NEW = 2, TE_NEW_ORPHANS = 3, TE_REACHED = 4, TE_ORPHANS = 5, TE_COPIES = 6, TE_FRESH = 7 };
enum { TY_ID = 0, TY_VAL = 1, TY_REACHED = 2, TY_ORPHANS = 3, TY_DEPTH = 4, TY_HOPS = 5, TY_MOST = 6, TY_MOST_ID = 7, TY_HOP_BIN = 8,
       TY_CH_BIN = TY_HOP_BIN + SIM_TREE_BINS };
// rows of the partial matrix an entry, and of the summary's pass
enum { TRW_NEW = 0, TRW_NEW_ORPHANS = 1, TRW_COPIES = 2, TRW_FRESH = 3 };
enum { TRY_REACHED = 0, TRY_ORPHANS = 1, TRY_DEPTH = 2, TRY_HOPS = 3, TRY_MOST = 4, TRY_BIN = 5, TRY_ROWS = TRY_BIN + 2 * SIM_TREE_BINS };

struct TreeDevP {
  const LedTab* tab;  // the entries: id, val = ltime, the index by (kind, key)
  u32* arrival;       // [n][Nl]: 0 = not yet
  u32* parent;        // [n][Nl]: frozen where arrival != 0; the candidate where cmask says so; scratch otherwise
  u32* hop;           // [n][Nl]: written where a node latches
  u64* have;          // [Nl]: bit e = arrival[e][l] != 0
  u64* cmask;         // [Nl]: bit e = parent[e][l] holds a candidate of the last sample
  u64* carry;         // [4][Nl]: bit e = the packet node l sent in this slot carries entry e
  u64* part;          // [1 + TREE_ROWS n][G]
  u64* out;           // the sample's slot: 8 + 8 n words
  const u64* prev;    // the previous sample's slot; null: this is the first
  Flight fl;          // the packets of the sampled tick, its graph's rows included
  u32 G;              // workgroups of the per-tick kernels
  u32 n;              // entries
  u32 now;            // sim_tick after the sampled tick
  u32 use_cand;       // the previous sample was taken and its stamp is now - 1
};

__global__ __launch_bounds__(BLOCK) void tree_latch_kernel(Dev d, const uint4* base, TreeDevP p) {
  __shared__ LedTab tab;
  __shared__ u32 cnt[SIM_TREE_MAX * 2];  // new, new orphans
  __shared__ u32 s_up;
  lds_stage(tab, p.tab);
  for (u32 i = threadIdx.x; i < SIM_TREE_MAX * 2; i += BLOCK) cnt[i] = 0;
  if (threadIdx.x == 0) s_up = 0;
  __syncthreads();
  const bool lane0 = (threadIdx.x & 63) == 0;
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together: the ballots below need every lane
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in = l < d.Nl;
    const bool up = in && (d.R1[l].z & SIM_RF_UP);
    const u64 mu = __ballot(up);
    if (lane0 && mu) atomicAdd(&s_up, (u32)__popcll(mu));  // (LDS)
    const u64 cm = in && p.use_cand ? p.cmask[l] : 0ull;
    u64 hv = 0;
    for (u32 e = 0; e < p.n; ++e) {
      const size_t at = (size_t)e * d.Nl + l;
      u32 a = in ? p.arrival[at] : 0u;
      const u64 id = tab.id[e];
      const bool latch = up && a == 0u && rumour_held(d, base, l, (u32)(id >> 32), (u32)id, tab.val[e]);
      bool orphan = false;
      if (latch) {
        u32 par = SIM_TREE_NONE, hp = 0;
        if ((cm >> e) & 1ull) {
          const u32 c = p.parent[at];  // the smallest sender among the carriers the last sample saw addressed to l
          if (c < d.Nl) {
            const u32 ac = p.arrival[(size_t)e * d.Nl + c];  // (a parent latching in this launch reads as 0 or as now)
            if (ac != 0u && ac < p.now) { par = c; hp = p.hop[(size_t)e * d.Nl + c] + 1u; }
          }
        }
        p.arrival[at] = p.now; p.parent[at] = par; p.hop[at] = hp;
        a = p.now;
        orphan = par == SIM_TREE_NONE;
      }
      if (a) hv |= 1ull << e;
      const u64 mn = __ballot(latch), mo = __ballot(orphan);
      if (lane0 && mn) atomicAdd(&cnt[e * 2], (u32)__popcll(mn));  // (LDS)
      if (lane0 && mo) atomicAdd(&cnt[e * 2 + 1], (u32)__popcll(mo));
    }
    if (in) p.have[l] = hv;
  }
  __syncthreads();
  // ---- the workgroup's column: row 0 the running nodes, then the latch's two rows of every entry ----
  if (threadIdx.x == 0) p.part[blockIdx.x] = s_up;
  for (u32 w = threadIdx.x; w < 2u * p.n; w += BLOCK)
    p.part[(size_t)(1u + (w >> 1) * TREE_ROWS + (w & 1u)) * p.G + blockIdx.x] = cnt[w];
}

__global__ __launch_bounds__(BLOCK) void tree_carry_kernel(Dev d, TreeDevP p) {
  struct Sent {  // sent_packets' visitor: a packet's carry mask, copied to every slot that maps to it; `copies` weighs by those slots
    const LedTab& tab;
    u32* cnt;
    u64 cm[SIM_MAX_FANOUT];  // (every index is a constant once the walk's loops are unrolled: registers)
    __device__ void page(u32 k, u32 wgt, const uint4* cell) {
      const uint4 ck = ld4(cell), cl = ld4(cell + 1), ch = ld4(cell + 2);
      const u32 kw[4] = {ck.x, ck.y, ck.z, ck.w}, lw[4] = {cl.x, cl.y, cl.z, cl.w}, hw[4] = {ch.x, ch.y, ch.z, ch.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u32 kind = SIM_META_KIND(hw[r]) & 7u;
        if (!kind) continue;  // (an empty record is all zero)
        const u32 e = ledger_find(tab, kind, kw[r], (u64)lw[r] | ((u64)(hw[r] >> 16) << 32));
        if (e == LED_NONE) continue;
        cm[k] |= 1ull << e;
        atomicAdd(&cnt[e], wgt);  // (LDS)
      }
    }
    __device__ void packet(u32, u32) {}
    __device__ void repeat(u32 k, u32 first) { cm[k] = cm[first]; }
  };
  __shared__ LedTab tab;
  __shared__ u32 cnt[SIM_TREE_MAX];  // copies
  lds_stage(tab, p.tab);
  if (threadIdx.x < SIM_TREE_MAX) cnt[threadIdx.x] = 0;
  __syncthreads();
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  for (size_t it = 0; it < passes; ++it) {
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (l >= d.Nl) continue;
    Sent v = {tab, cnt, {0, 0, 0, 0}};
    sent_packets(d, p.fl.cur, p.fl.nslot, l, v);
#pragma unroll
    for (u32 k = 0; k < SIM_MAX_FANOUT; ++k) p.carry[(size_t)k * d.Nl + l] = v.cm[k];
  }
  __syncthreads();
  for (u32 e = threadIdx.x; e < p.n; e += BLOCK) p.part[(size_t)(1u + e * TREE_ROWS + TRW_COPIES) * p.G + blockIdx.x] = cnt[e];
}

// ptp: the parameters of the tick that sent the packets (the bijection's map; unused under kRandomNodes)
__global__ __launch_bounds__(BLOCK) void tree_cand_kernel(Dev d, TickP ptp, TreeDevP p) {
  __shared__ u32 cnt[SIM_TREE_MAX];  // fresh
  if (threadIdx.x < SIM_TREE_MAX) cnt[threadIdx.x] = 0;
  __syncthreads();
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  for (size_t it = 0; it < passes; ++it) {
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (l >= d.Nl) continue;
    const u64 open = ~p.have[l];
    const bool up = d.R1[l].z & SIM_RF_UP;
    u64 seen = 0;
    const auto take = [&](u32 s, u32 k) {  // the packet sender s keeps for slot k: one 8-byte gather
      u64 b = p.carry[(size_t)k * d.Nl + s] & open;
      while (b) {
        const u32 e = (u32)__ffsll((unsigned long long)b) - 1u;
        b &= b - 1ull;
        u32* c = p.parent + (size_t)e * d.Nl + l;  // this node's own candidate
        if (!((seen >> e) & 1ull) || s < *c) *c = s;
        seen |= 1ull << e;
        if (up) atomicAdd(&cnt[e], 1u);  // (LDS)
      }
    };
    recv_packets(d, ptp, p.fl, l, take);
    p.cmask[l] = seen;
  }
  __syncthreads();
  for (u32 e = threadIdx.x; e < p.n; e += BLOCK) p.part[(size_t)(1u + e * TREE_ROWS + TRW_FRESH) * p.G + blockIdx.x] = cnt[e];
}

// one wave per word of the sample; written into the sample's slot
__global__ __launch_bounds__(BLOCK) void tree_fold_kernel(TreeDevP p) {
  const u32 w = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= SIM_TREE_HEADER_WORDS + SIM_TREE_ENTRY_WORDS * p.n) return;  // (whole waves)
  const auto row = [&](u32 e, u32 r) { return fold_row(p.part + (size_t)(1u + e * TREE_ROWS + r) * p.G, p.G, FOLD_SUM); };
  u64 v = 0;
  if (w < SIM_TREE_HEADER_WORDS) {
    if (w == TH_TICK) v = p.now;
    else if (w == TH_N) v = p.n;
    else if (w == TH_UP) v = fold_row(p.part, p.G, FOLD_SUM);
    else if (w >= TH_NEW && w <= TH_FRESH) { for (u32 e = 0; e < p.n; ++e) v += row(e, w - TH_NEW); }
  } else {
    const u32 i = (w - SIM_TREE_HEADER_WORDS) / SIM_TREE_ENTRY_WORDS, c = (w - SIM_TREE_HEADER_WORDS) % SIM_TREE_ENTRY_WORDS;
    if (c == TE_ID) v = p.tab->id[i];
    else if (c == TE_VAL) v = p.tab->val[i];
    else if (c == TE_NEW || c == TE_NEW_ORPHANS) v = row(i, c - TE_NEW);
    else if (c == TE_REACHED || c == TE_ORPHANS) v = row(i, c - TE_REACHED) + (p.prev ? p.prev[w] : 0ull);
    else v = row(i, TRW_COPIES + (c - TE_COPIES));
  }
  if (!lane) p.out[w] = v;
}

// ---- the reads ----
// one entry's planes: children[parent[l]] += 1 for every node with a parent (ch zeroed beforehand)
__global__ __launch_bounds__(BLOCK) void tree_children_kernel(const u32* arrival, const u32* parent, u32 Nl, u32* ch) {
  for (size_t l = (size_t)blockIdx.x * BLOCK + threadIdx.x; l < Nl; l += (size_t)gridDim.x * BLOCK) {
    const u32 par = arrival[l] ? parent[l] : SIM_TREE_NONE;
    if (par < Nl) atomicAdd(&ch[par], 1u);
  }
}
// nodes first .. first + count - 1 of one entry's planes into their 16-byte records
__global__ __launch_bounds__(BLOCK) void tree_links_kernel(const u32* arrival, const u32* parent, const u32* hop, const u32* ch, u32 first,
                                                           u32 count, uint4* out) {
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= count) return;
  const u32 a = arrival[first + i];
  out[i] = make_uint4(a, a ? parent[first + i] : SIM_TREE_NONE, a ? hop[first + i] : 0u, ch[first + i]);
}

struct TreeStatP {
  const u32 *arrival, *parent, *hop, *ch;  // one entry's planes [Nl] and the children counted on scratch
  const LedTab* tab;
  u64* part;  // [TRY_ROWS][G]
  u64* out;   // the entry's 72 words
  u32 G, entry;
};
__global__ __launch_bounds__(BLOCK) void tree_stat_kernel(u32 Nl, TreeStatP p) {
  __shared__ unsigned long long acc[TRY_BIN];
  __shared__ u32 bins[2 * SIM_TREE_BINS];
  if (threadIdx.x < TRY_BIN) acc[threadIdx.x] = 0;
  if (threadIdx.x < 2 * SIM_TREE_BINS) bins[threadIdx.x] = 0;
  __syncthreads();
  u64 hops = 0, key = 0, depth = 0;
  u32 reached = 0, orphans = 0;
  for (size_t l = (size_t)blockIdx.x * BLOCK + threadIdx.x; l < Nl; l += (size_t)gridDim.x * BLOCK) {
    if (!p.arrival[l]) continue;
    const u32 hp = p.hop[l], c = p.ch[l];
    reached++;
    orphans += p.parent[l] == SIM_TREE_NONE ? 1u : 0u;
    hops += hp;
    depth = max(depth, (u64)hp);
    key = max(key, ((u64)c << 32) | (u64)(~(u32)l));
    atomicAdd(&bins[min(hp, SIM_TREE_BINS - 1u)], 1u);  // (LDS)
    atomicAdd(&bins[SIM_TREE_BINS + min(c, SIM_TREE_BINS - 1u)], 1u);
  }
  lds_sum(&acc[TRY_REACHED], reached);
  lds_sum(&acc[TRY_ORPHANS], orphans);
  lds_max(&acc[TRY_DEPTH], depth);
  lds_sum(&acc[TRY_HOPS], hops);
  lds_max(&acc[TRY_MOST], key);
  __syncthreads();
  if (threadIdx.x < TRY_ROWS)
    p.part[(size_t)threadIdx.x * p.G + blockIdx.x] = threadIdx.x < TRY_BIN ? (u64)acc[threadIdx.x] : (u64)bins[threadIdx.x - TRY_BIN];
}
// one wave per word of the entry's summary
__global__ __launch_bounds__(BLOCK) void tree_stat_fold(TreeStatP p) {
  const u32 w = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= SIM_TREE_SUMMARY_WORDS) return;  // (whole waves)
  const auto row = [&](u32 r, u32 op) { return fold_row(p.part + (size_t)r * p.G, p.G, op); };
  u64 v;
  if (w == TY_ID) v = p.tab->id[p.entry];
  else if (w == TY_VAL) v = p.tab->val[p.entry];
  else if (w == TY_REACHED) v = row(TRY_REACHED, FOLD_SUM);
  else if (w == TY_ORPHANS) v = row(TRY_ORPHANS, FOLD_SUM);
  else if (w == TY_DEPTH) v = row(TRY_DEPTH, FOLD_MAX);
  else if (w == TY_HOPS) v = row(TRY_HOPS, FOLD_SUM);
  else if (w == TY_MOST) v = row(TRY_MOST, FOLD_MAX) >> 32;
  else if (w == TY_MOST_ID) { const u64 k = row(TRY_MOST, FOLD_MAX); v = k ? (u64)(~(u32)k) : 0ull; }  // (a reached node's key is never 0)
  else v = row(TRY_BIN + (w - TY_HOP_BIN), FOLD_SUM);
  if (!lane) p.out[w] = v;
}

// one lane: node, parent, grandparent ... — hop + 1 ids, the first `room` of them into ids[], the number of all into ids[room]
__global__ void tree_path_kernel(const u32* arrival, const u32* parent, const u32* hop, u32 Nl, u32 node, u32* ids, u32 room) {
  if (blockIdx.x || threadIdx.x) return;
  const u32 total = arrival[node] ? hop[node] + 1u : 0u;
  u32 at = node, i = 0;
  for (; i < total && at < Nl; ++i) {  // (hop + 1 <= Nl: arrivals strictly fall along the chain)
    if (i < room) ids[i] = at;
    at = parent[at];
  }
  ids[room] = i;
}

struct TreeTopP {
  const u32 *arrival, *parent, *hop, *ch;
  u64* ckey;  // [G][top_k]: a workgroup's candidates, descending; 0 ends a shorter list
  u64* crec;  // [G][top_k][TREE_RANK_WORDS]: their records
  u64* top;   // [top_k][TREE_RANK_WORDS]
  u32 G;      // workgroups of the top kernel: ceil(Nl / BLOCK)
  u32 top_k;
};
__global__ __launch_bounds__(BLOCK) void tree_top_kernel(Dev d, TreeTopP p) {
  __shared__ u64 red[2][BLOCK / 64];
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;  // the node
  const bool in = i < d.Nl;
  const u32 a = in ? p.arrival[i] : 0u;
  const u32 par = a ? p.parent[i] : SIM_TREE_NONE, hp = a ? p.hop[i] : 0u, c = in ? p.ch[i] : 0u;
  const bool up = in && (d.R1[in ? i : 0u].z & SIM_RF_UP);
  const u64 w[TREE_RANK_WORDS] = {(u64)i | ((u64)(up ? 1u : 0u) << 32), (u64)a | ((u64)par << 32), (u64)hp | ((u64)c << 32)};
  // i < 2^24: a node's key is never 0
  const u64 key = in ? ((u64)c << 32) | (u64)(0xFFFFFFFFu - i) : 0ull;
  rank_candidates<TREE_RANK_WORDS>(key, w, p.ckey, p.crec, p.top_k, red);
}
// one workgroup: the lists merged; records beyond the nodes get id 0xFFFFFFFF and zeros
__global__ __launch_bounds__(BLOCK) void tree_top_fold(TreeTopP p) {
  __shared__ u64 red[2][BLOCK / 64];
  rank_merge<TREE_RANK_WORDS>(p.ckey, p.crec, p.G, p.top_k, p.top, red, FillNoId());
}

// ---- host ----
static inline size_t tree_stride(u32 n) { return SIM_TREE_HEADER_WORDS + (size_t)n * SIM_TREE_ENTRY_WORDS; }  // words of a sample
static inline u32 tree_grid(const sim_handle* h) { return (u32)std::min<size_t>(((size_t)h->d.Nl + BLOCK - 1) / BLOCK, TREE_GRID); }

// the entries checked (the spread map's rules) and put into the ledger's table, index included; touches nothing but t
static int tree_check(const sim_handle* h, const sim_tree_entry* e, u32 n, LedTab& t) {
  SprTab st;
  if (int rc = spread_check(h, e, n, st)) return rc;
  ConvSet cs;
  return ledger_check(h, reinterpret_cast<const sim_ledger_entry*>(e), n, t, cs);  // (the same layout: the static_assert above)
}

struct TreeState : Observer {  // samples of 8 + 8 n words
  DevScratch<LedTab> d_tab;
  DevScratch<u32> d_planes;  // arrival, parent, hop: [3][n][Nl]
  DevScratch<u64> d_masks;   // have, cmask, carry: [2 + 4][Nl]
  DevScratch<u64> d_part;    // [1 + TREE_ROWS n][TREE_GRID]
  u32 n = 0;
  u64 stamp = ~0ull;         // the `now` of the last sample taken — its candidates' stamp —; none yet
  u32* arrival(const sim_handle* h) const { return d_planes.get(); }
  u32* parent(const sim_handle* h) const { return d_planes.get() + (size_t)n * h->d.Nl; }
  u32* hop(const sim_handle* h) const { return d_planes.get() + (size_t)2 * n * h->d.Nl; }
  // checks, then the ring planes the predicate reads (the route sim_track_add takes), the planes (zeroed on the stream) and the table's upload
  int setup(sim_handle* h, const sim_tree_entry* e, u32 cnt) {
    LedTab t;
    if (int rc = tree_check(h, e, cnt, t)) return rc;
    for (u32 i = 0; i < cnt; ++i)
      if (int rc = conv_plane(h, e[i].kind, e[i].ltime)) return rc;
    n = cnt;
    const size_t Nl = h->d.Nl;
    if (int rc = d_tab.alloc(1)) return rc;
    if (int rc = d_planes.alloc((size_t)3 * n * Nl)) return rc;
    if (int rc = d_masks.alloc((size_t)(2 + SIM_MAX_FANOUT) * Nl)) return rc;
    if (int rc = d_part.alloc((1u + (size_t)TREE_ROWS * n) * TREE_GRID)) return rc;
    HCHECK(hipMemcpy(d_tab.get(), &t, sizeof t, hipMemcpyHostToDevice));
    HCHECK(hipMemsetAsync(d_planes.get(), 0, (size_t)3 * n * Nl * 4, h->stream));
    HCHECK(hipMemsetAsync(d_masks.get(), 0, (size_t)(2 + SIM_MAX_FANOUT) * Nl * 8, h->stream));
    return SIM_OK;
  }
  int sample(sim_handle* h, u64* out) override {
    const Dev& d = h->d;
    TreeDevP p;
    p.tab = d_tab.get();
    p.arrival = arrival(h); p.parent = parent(h); p.hop = hop(h);
    p.have = d_masks.get(); p.cmask = p.have + d.Nl; p.carry = p.have + (size_t)2 * d.Nl;
    p.part = d_part.get(); p.out = out;
    p.prev = smp.taken ? out - smp.stride_words : nullptr;
    if (int rc = flight_fill(h, true, p.fl)) return rc;
    p.G = tree_grid(h);
    p.n = n;
    p.now = (u32)h->tick;
    p.use_cand = stamp + 1 == h->tick ? 1u : 0u;
    tree_latch_kernel<<<p.G, BLOCK, 0, h->stream>>>(d, h->d_base, p);
    tree_carry_kernel<<<p.G, BLOCK, 0, h->stream>>>(d, p);
    tree_cand_kernel<<<p.G, BLOCK, 0, h->stream>>>(d, h->prev, p);
    const u32 words = (u32)tree_stride(n);
    tree_fold_kernel<<<(words + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    stamp = h->tick;
    return SIM_OK;
  }
};
static inline TreeState* tree_of(const sim_handle* h) { return static_cast<TreeState*>(h->obs[OB_TREE]); }

// one entry's children counted into ch[Nl] (zeroed here, on the stream)
static int tree_children_launch(sim_handle* h, const TreeState* s, u32 entry, u32* ch) {
  const size_t Nl = h->d.Nl;
  HCHECK(hipMemsetAsync(ch, 0, std::max<size_t>(Nl, 1) * 4, h->stream));
  tree_children_kernel<<<tree_grid(h), BLOCK, 0, h->stream>>>(s->arrival(h) + entry * Nl, s->parent(h) + entry * Nl, (u32)Nl, ch);
  HCHECK(hipGetLastError());
  return SIM_OK;
}

extern "C" {

uint32_t sim_tree_version(void) { return SIM_TREE_VERSION; }

int sim_tree_start(sim_handle* h, const sim_tree_entry* e, uint32_t n, uint32_t first_tick, uint32_t capacity) {
  TreeState* s = new TreeState();
  const auto check = [&] {
    LedTab t;
    return tree_check(h, e, n, t);
  };
  return observer_start(h, OB_TREE, s, SIM_TREE_MAX_SAMPLES, first_tick, 1u, capacity, tree_stride(n), check, [&] { return s->setup(h, e, n); });
}

int sim_tree_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_TREE, taken, dropped); }

int sim_tree_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_TREE, first, n, out, cap_words, n_out);
}

int sim_tree_stop(sim_handle* h) { return observer_stop(h, OB_TREE); }

int sim_tree_links(sim_handle* h, uint32_t entry, uint32_t first_node, uint32_t count, sim_tree_link* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out || (u64)first_node + count > h->d.N) return SIM_EINVAL;
  const TreeState* s = tree_of(h);
  if (!s) return SIM_ESTATE;
  if (entry >= s->n) return SIM_EINVAL;
  const size_t Nl = h->d.Nl;
  DevScratch<u32> d_ch;
  DevScratch<uint4> d_out;
  if (int rc = d_ch.alloc(Nl)) return rc;
  if (int rc = d_out.alloc(count)) return rc;
  int rc = observer_settle(h, [&]() -> int {
    if (!count) return SIM_OK;
    if (int lrc = tree_children_launch(h, s, entry, d_ch.get())) return lrc;
    tree_links_kernel<<<(count + BLOCK - 1) / BLOCK, BLOCK, 0, h->stream>>>(s->arrival(h) + entry * Nl, s->parent(h) + entry * Nl,
                                                                            s->hop(h) + entry * Nl, d_ch.get(), first_node, count, d_out.get());
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
  if (rc != SIM_OK) return rc;
  if (count) HCHECK(hipMemcpy(out, d_out.get(), (size_t)count * sizeof *out, hipMemcpyDeviceToHost));
  return SIM_OK;
}

int sim_tree_summary(sim_handle* h, uint64_t* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out) return SIM_EINVAL;
  const TreeState* s = tree_of(h);
  if (!s) return SIM_ESTATE;
  const size_t Nl = h->d.Nl, words = (size_t)s->n * SIM_TREE_SUMMARY_WORDS;
  DevScratch<u32> d_ch;
  DevScratch<u64> part, d_out;
  if (int rc = d_ch.alloc(Nl)) return rc;
  if (int rc = part.alloc((size_t)TRY_ROWS * tree_grid(h))) return rc;
  if (int rc = d_out.alloc(words)) return rc;
  int rc = observer_settle(h, [&]() -> int {
    for (u32 e = 0; e < s->n; ++e) {  // (the stream's order lets every entry use the same scratch)
      if (int lrc = tree_children_launch(h, s, e, d_ch.get())) return lrc;
      TreeStatP p;
      p.arrival = s->arrival(h) + e * Nl; p.parent = s->parent(h) + e * Nl; p.hop = s->hop(h) + e * Nl; p.ch = d_ch.get();
      p.tab = s->d_tab.get(); p.part = part.get(); p.out = d_out.get() + (size_t)e * SIM_TREE_SUMMARY_WORDS;
      p.G = tree_grid(h);
      p.entry = e;
      tree_stat_kernel<<<p.G, BLOCK, 0, h->stream>>>((u32)Nl, p);
      tree_stat_fold<<<(SIM_TREE_SUMMARY_WORDS + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
      HCHECK(hipGetLastError());
    }
    return SIM_OK;
  });
  if (rc != SIM_OK) return rc;
  HCHECK(hipMemcpy(out, d_out.get(), words * 8, hipMemcpyDeviceToHost));
  return SIM_OK;
}

int sim_tree_path(sim_handle* h, uint32_t entry, uint32_t node, uint32_t* ids, uint32_t cap, uint32_t* n_out, uint32_t* total) {
  if (int rc = observer_usable(h)) return rc;
  if (!n_out || !total || (cap && !ids) || node >= h->d.N) return SIM_EINVAL;
  const TreeState* s = tree_of(h);
  if (!s) return SIM_ESTATE;
  if (entry >= s->n) return SIM_EINVAL;
  const size_t Nl = h->d.Nl;
  return observer_read_ids(h, ids, cap, n_out, total, [&](u32* d_ids, u32 room, u32*) -> int {  // (the kernel puts the total behind the ids)
    tree_path_kernel<<<1, 64, 0, h->stream>>>(s->arrival(h) + entry * Nl, s->parent(h) + entry * Nl, s->hop(h) + entry * Nl, (u32)Nl, node,
                                              d_ids, room);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
}

int sim_tree_top(sim_handle* h, uint32_t entry, uint32_t top_k, sim_tree_rank* ranks) {
  if (int rc = observer_usable(h)) return rc;
  if (!ranks || !top_k || top_k > SIM_TREE_TOP_MAX) return SIM_EINVAL;
  const TreeState* s = tree_of(h);
  if (!s) return SIM_ESTATE;
  if (entry >= s->n) return SIM_EINVAL;
  const size_t Nl = h->d.Nl;
  DevScratch<u32> d_ch;
  if (int rc = d_ch.alloc(Nl)) return rc;
  return observer_read_top(h, top_k, 1u, TREE_RANK_WORDS, ranks, [&](u64* ckey, u64* crec, u64* d_top, u32 G) -> int {
    if (int lrc = tree_children_launch(h, s, entry, d_ch.get())) return lrc;
    TreeTopP p;
    p.arrival = s->arrival(h) + entry * Nl; p.parent = s->parent(h) + entry * Nl; p.hop = s->hop(h) + entry * Nl; p.ch = d_ch.get();
    p.ckey = ckey; p.crec = crec; p.top = d_top;
    p.G = G;
    p.top_k = top_k;
    tree_top_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d, p);
    tree_top_fold<<<1, BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
}

}  // extern "C"
