// serf_sim_catalog.inc — part of the translation unit serf_sim.hip (included from there, behind the query board; not a header of its own).
// Rumour catalogue (include/serf_sim_catalog.h): three kernels behind a sampled tick's last launch, the host's bookkeeping, the entry points.
//
// The set of live identities is not known in advance, so there is no table to stage.  It is BUILT, a table per wave in LDS that only its
// wave touches: no hash table shared between waves, no lock, no compare-and-swap loop, no atomics on global memory.
//
// Per sampled tick:
//   catalog_scan_kernel   the ledger's layout (ledger_count_kernel): a node per lane, grid-stride, CATALOG_GRID workgroups at most, whole
//                         waves kept together, the same loads of R1 / R2, qkeys, qpay and q_count.  Every wave owns a CatTab of
//                         SIM_CATALOG_LIVE places {id, val, holders, queued, transmits, in flight, fresh} in LDS (36 bytes a place, 36 KiB a
//                         workgroup).  Insertion is cooperative and wave-uniform (cat_add): the wave takes the identity of its first lane
//                         that still has an unjudged record at the current position (ballot, shuffle), all 64 lanes compare it with
//                         place[lane + 64 r] for the rounds r the table's fill needs (cat_place), a ballot finds the place or the next free
//                         one is taken, every lane whose record matches adds its share through ONE wave sum of packed fields, and those
//                         lanes retire.  Holders count a node once: a 256-bit mask of the places a lane has counted.  Every lane of the
//                         wave takes part in every ballot: the loops over queue positions run to the wave's deepest queue, lanes beyond
//                         their own depth are predicated off.  The sent_packets visitor runs in divergent code, so it only NOTES where a
//                         node's distinct packets lie (first cell, pages, weight per fan-out slot); the cells are loaded and judged in a loop
//                         every lane runs.  A table that fills sets the overflow flag and drops the identity.  At the end wave 0 merges
//                         the other waves' tables into its own (cat_merge_from, behind a barrier) and the workgroup writes table, fill
//                         and flag into its slab and its column of the header sums
//   catalog_merge_kernel  fan-in CAT_FANIN: workgroup g merges tables 32 g .. 32 g + 31 into one — eight a wave, then wave 0 the four —
//                         launched again until one table is left: two levels at most for 1 024 tables.  The flags are OR-ed.  Every table
//                         is a subset of the cluster's set: none overflows unless that set exceeds SIM_CATALOG_LIVE, and beyond it the
//                         last merge must — word 3 is exactly "distinct > 256", whatever the grid
//   catalog_fold_kernel   one workgroup, a thread per place: ranks the final table in ascending (id, val) by a count of smaller keys in
//                         LDS, writes the live table, matches it against the registry (a thread per registry record, a binary search in
//                         the ranked table), updates last-seen, peaks and sums, counts died and revived against the previous good sample
//                         (its set and its stamp are kept on the device), appends the unmatched identities in rank order up to max_ids,
//                         folds the header rows (fold_row) and writes the sample
// Their order is the stream's.  The host knows every sampled tick in advance: it passes the slot to the launches and reads nothing back.
// A handle without a started catalogue never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_catalog.h"

#define CATALOG_GRID 1024u  // workgroups of the scan kernel at most
#define CAT_FANIN 32u       // tables one workgroup of the merge kernel takes
#define CAT_NONE 0xFFFFFFFFu
#define CAT_CNT 5u          // counters a place: words 3 .. 7 of a live entry
enum { CC_HOLD = 0, CC_QUEUED = 1, CC_TX = 2, CC_FLIGHT = 3, CC_FRESH = 4 };
enum { CR_UP = 0, CR_QUEUED = 1, CR_FLIGHT = 2, CR_PKTS = 3, CR_TX = 4, CR_ROWS = 5 };  // rows of the partial matrix: words 1, 9 .. 12
// words of a sample
enum { CAW_TICK = 0, CAW_UP = 1, CAW_LIVE = 2, CAW_OVF = 3, CAW_NEW = 4, CAW_DIED = 5, CAW_REVIVED = 6, CAW_REG = 7, CAW_LOST = 8, CAW_QUEUED = 9,
       CAW_FLIGHT = 10, CAW_PKTS = 11, CAW_TX = 12, CAW_KIND_IDS = 13, CAW_KIND_QUEUED = 20, CAW_KIND_FLIGHT = 27, CAW_OVERFLOWED = 34 };
// what a running catalogue keeps on the device besides registry, stamps and the previous good sample's live table
enum { CS_REG = 0, CS_LOST = 1, CS_OVERFLOWED = 2, CS_SEQ = 3, CS_LIVE_N = 4, CS_PREV_N = 5, CS_WORDS = 8 };
static_assert(SIM_CATALOG_LIVE == 256u && SIM_CATALOG_LIVE == BLOCK && SIM_CATALOG_SAMPLE_WORDS == 48u && SIM_CATALOG_RECORD_WORDS == 8u &&
              CAT_FANIN % (BLOCK / 64) == 0, "layout of include/serf_sim_catalog.h; the fold has a thread per place; a holder mask of 4 x 64 bits");

struct CatTab {  // one wave's (LDS), one workgroup's (a slab in global memory)
  u64 id[SIM_CATALOG_LIVE];
  u64 val[SIM_CATALOG_LIVE];
  u32 c[CAT_CNT][SIM_CATALOG_LIVE];
};
struct CatSlab {
  CatTab t;
  u32 fill, ovf, pad[2];
};

__device__ static inline u64 cat_identity_val(u32 kind, u64 val) { return SIM_WIRE_TWO_PART(kind) ? (val & 0xFFFFFFull) : (val & 0xFFFFFFFFFFFFull); }
__device__ static inline bool cat_less(u64 ia, u64 va, u64 ib, u64 vb) { return ia < ib || (ia == ib && va < vb); }

// The place of identity (cid, cval) — the same in every lane — in the calling wave's table: found, or the next free one taken and zeroed,
// or CAT_NONE with the flag set when the table is full.  Every lane of the wave calls it; fill and ovf are the same in every lane
__device__ static inline u32 cat_place(CatTab& t, u32& fill, u32& ovf, u32 lane, u64 cid, u64 cval) {
  u32 place = CAT_NONE;
  for (u32 r = 0; 64u * r < fill && place == CAT_NONE; ++r) {
    const u32 p = lane + 64u * r;
    const u64 hit = __ballot(p < fill && t.id[p] == cid && t.val[p] == cval);
    if (hit) place = 64u * r + (u32)__ffsll((unsigned long long)hit) - 1u;
  }
  if (place != CAT_NONE) return place;
  if (fill >= SIM_CATALOG_LIVE) { ovf = 1u; return CAT_NONE; }
  place = fill++;
  if (lane == 0) {
    t.id[place] = cid; t.val[place] = cval;
#pragma unroll
    for (u32 k = 0; k < CAT_CNT; ++k) t.c[k][place] = 0;
  }
  __builtin_amdgcn_wave_barrier();  // (one wave, LDS in order: the next round's compare reads what lane 0 wrote)
  return place;
}
// The records of one position, one per lane at most (have), into the wave's table.  A lane's share: q queued (0 / 1), tx transmits
// (< 64), fl in-flight copies (<= SIM_MAX_FANOUT), fr fresh (0 / 1); hold: the record lies in the lane's queue — the lane is counted
// as a holder of the place unless `held` says it has been.  A round takes 64 shares at most: the fields of the packed sum cannot carry
__device__ static inline void cat_add(CatTab& t, u32& fill, u32& ovf, u32 lane, bool have, u64 id, u64 val, u32 q, u32 tx, u32 fl, u32 fr,
                                      bool hold, u64 (&held)[4]) {
  for (;;) {
    const u64 pend = __ballot(have);
    if (!pend) break;
    const int src = __ffsll((unsigned long long)pend) - 1;
    const u64 cid = __shfl(id, src), cval = __shfl(val, src);
    const u32 place = cat_place(t, fill, ovf, lane, cid, cval);
    const bool mine = have && id == cid && val == cval;
    if (place != CAT_NONE) {  // (the same in every lane)
      u32 h = 0;
      const u64 bit = 1ull << (place & 63u);
#pragma unroll
      for (u32 k = 0; k < 4; ++k)
        if ((place >> 6) == k && mine && hold) { h = (held[k] & bit) ? 0u : 1u; held[k] |= bit; }
      const u64 sum = wave_sum(mine ? ((u64)q | ((u64)fr << 8) | ((u64)h << 16) | ((u64)tx << 24) | ((u64)fl << 40)) : 0ull);
      if (lane == 0) {
        t.c[CC_QUEUED][place] += (u32)(sum & 0xFFu);
        t.c[CC_FRESH][place] += (u32)((sum >> 8) & 0xFFu);
        t.c[CC_HOLD][place] += (u32)((sum >> 16) & 0xFFu);
        t.c[CC_TX][place] += (u32)((sum >> 24) & 0xFFFFu);
        t.c[CC_FLIGHT][place] += (u32)((sum >> 40) & 0xFFFFu);
      }
    }
    have = have && !mine;
  }
}
// Table s (sfill places; in LDS or in a slab) into the wave's: the same routine, a place per lane.  The identities of ONE table are
// distinct, so a round has one lane, which adds its counters whole
__device__ static inline void cat_merge_from(CatTab& t, u32& fill, u32& ovf, u32 lane, const CatTab& s, u32 sfill) {
  for (u32 base = 0; base < sfill; base += 64u) {  // (the same in every lane)
    const u32 p = base + lane;
    bool have = p < sfill;
    const u64 id = have ? s.id[p] : 0ull, val = have ? s.val[p] : 0ull;
    u32 c[CAT_CNT];
#pragma unroll
    for (u32 k = 0; k < CAT_CNT; ++k) c[k] = have ? s.c[k][p] : 0u;
    for (;;) {
      const u64 pend = __ballot(have);
      if (!pend) break;
      const u32 src = (u32)__ffsll((unsigned long long)pend) - 1u;
      const u32 place = cat_place(t, fill, ovf, lane, __shfl(id, (int)src), __shfl(val, (int)src));
      if (place != CAT_NONE && lane == src) {
#pragma unroll
        for (u32 k = 0; k < CAT_CNT; ++k) t.c[k][place] += c[k];
      }
      __builtin_amdgcn_wave_barrier();
      have = have && lane != src;
    }
  }
}
// The end of a workgroup of the scan and of the merge: wave 0 merges the other waves' tables into its own, the workgroup writes it
__device__ static inline void cat_group_write(CatTab* tabs, u32* fills, u32* ovfs, u32 fill, u32 ovf, CatSlab* out) {
  const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (lane == 0) { fills[wave] = fill; ovfs[wave] = ovf; }
  __syncthreads();
  if (wave == 0) {
    for (u32 w = 1; w < BLOCK / 64; ++w) {
      ovf |= ovfs[w];
      cat_merge_from(tabs[0], fill, ovf, lane, tabs[w], fills[w]);
    }
    if (lane == 0) { fills[0] = fill; ovfs[0] = ovf; }
  }
  __syncthreads();
  const u32 n = fills[0];
  for (u32 p = threadIdx.x; p < n; p += BLOCK) {
    out->t.id[p] = tabs[0].id[p]; out->t.val[p] = tabs[0].val[p];
#pragma unroll
    for (u32 k = 0; k < CAT_CNT; ++k) out->t.c[k][p] = tabs[0].c[k][p];
  }
  if (threadIdx.x == 0) { out->fill = n; out->ovf = ovfs[0]; }
}

struct CatScanP {
  CatSlab* slab;  // [G]: every workgroup writes its table
  u64* part;      // [CR_ROWS][G]: and its column of the header sums
  u32 G;
  u32 mask;       // kinds catalogued
  Flight fl;      // the packets in flight (cur and nslot: the catalogue reads no rows)
};

__global__ __launch_bounds__(BLOCK) void catalog_scan_kernel(Dev d, CatScanP p) {
  struct Note {  // sent_packets' visitor, in divergent code: where the node's distinct packets lie, per fan-out slot — nothing is judged here
    const uint4* first[SIM_MAX_FANOUT];
    u32 pages[SIM_MAX_FANOUT], wgt[SIM_MAX_FANOUT];  // (every index is a constant once the walk's loops are unrolled: registers)
    __device__ void page(u32 k, u32 w, const uint4* cell) {
      if (!pages[k]) first[k] = cell;
      pages[k]++;
      wgt[k] = w;
    }
    __device__ void packet(u32, u32) {}
    __device__ void repeat(u32, u32) {}
  };
  __shared__ CatTab tabs[BLOCK / 64];
  __shared__ u32 fills[BLOCK / 64], ovfs[BLOCK / 64];
  __shared__ unsigned long long hdr[CR_ROWS];
  if (threadIdx.x < CR_ROWS) hdr[threadIdx.x] = 0;
  __syncthreads();
  const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  CatTab& tab = tabs[wave];
  u32 fill = 0, ovf = 0;                              // the same in every lane of the wave
  u32 c_up = 0;                                       // a ballot per pass (the same value in every lane)
  u32 q_all = 0, tx_all = 0, fl_all = 0, pkts = 0;    // per lane, reduced over the wave once, at the end
  const size_t cell_u4 = d.rfan ? RF_CELL_U4 : PK_U4, page_u4 = (size_t)d.Nl * cell_u4;  // a packet's pages lie Nl cells apart
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together: the ballots below need every lane
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in = l < d.Nl;
    uint4 r1 = make_uint4(0, 0, 0, 0), r2 = r1;
    if (in) { r1 = ld4(&d.R1[l]); r2 = ld4(&d.R2[l]); }
    const bool up = in && (r1.z & SIM_RF_UP);
    c_up += (u32)__popcll(__ballot(up));
    u64 held[4] = {0ull, 0ull, 0ull, 0ull};  // the places this node has been counted a holder of
    // ---- the queues: position by position up to the wave's deepest; a lane beyond its own depth loads nothing and offers nothing ----
    const u32 depth = up ? q_count(d, l, r2.z) : 0u;
    const u32 deepest = (u32)wave_max(depth);
    for (u32 g = 0; 4u * g < deepest; ++g) {
      uint4 k4 = make_uint4(0, 0, 0, 0);
      if (4u * g < depth) k4 = ld4(&d.qkeys[(size_t)g * d.Nl + l]);
      const u32 kk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
      for (u32 j = 0; j < 4; ++j) {
        const bool act = 4u * g + j < depth;
        uint4 pay = make_uint4(0, 0, 0, 0);
        if (act) pay = ld4(&d.qpay[(size_t)(kk[j] & QK_SLOT_MASK) * d.Nl + l]);
        const u32 tx = act ? (kk[j] >> QK_TX_SH) & 0x3Fu : 0u;  // SIM_META_TRANSMITS of the canonical record
        tx_all += tx;
        const u32 kind = SIM_META_KIND(pay.y);
        cat_add(tab, fill, ovf, lane, act && ((p.mask >> kind) & 1u), (u64)pay.x | ((u64)kind << 32),
                cat_identity_val(kind, (u64)pay.z | ((u64)pay.w << 32)), 1u, tx, 0u, tx ? 0u : 1u, true, held);
      }
    }
    q_all += depth;
    // ---- the packets this node sent last tick: noted where they lie, then page by page up to the wave's longest ----
    Note v = {};
    if (in) sent_packets(d, p.fl.cur, p.fl.nslot, l, v);
#pragma unroll
    for (u32 k = 0; k < SIM_MAX_FANOUT; ++k) {
      const u32 longest = (u32)wave_max(v.pages[k]);
      u32 any = 0;
      for (u32 pg = 0; pg < longest; ++pg) {
        uint4 ck = make_uint4(0, 0, 0, 0), cl = ck, ch = ck;  // (an empty record is all zero)
        if (pg < v.pages[k]) {
          const uint4* cell = v.first[k] + (size_t)pg * page_u4;
          ck = ld4(cell); cl = ld4(cell + 1); ch = ld4(cell + 2);
        }
        const u32 kw[4] = {ck.x, ck.y, ck.z, ck.w}, lw[4] = {cl.x, cl.y, cl.z, cl.w}, hw[4] = {ch.x, ch.y, ch.z, ch.w};
#pragma unroll
        for (u32 r = 0; r < 4; ++r) {
          const u32 kind = SIM_META_KIND(hw[r]) & 7u;
          any |= kind;
          fl_all += kind ? v.wgt[k] : 0u;
          cat_add(tab, fill, ovf, lane, kind && ((p.mask >> kind) & 1u), (u64)kw[r] | ((u64)kind << 32),
                  cat_identity_val(kind, (u64)lw[r] | ((u64)(hw[r] >> 16) << 32)), 0u, 0u, v.wgt[k], 0u, false, held);
        }
      }
      pkts += any ? v.wgt[k] : 0u;
    }
  }
  // ---- the workgroup's column and its table ----
  {
    const u64 s[4] = {q_all, fl_all, pkts, tx_all};
    const u32 sw[4] = {CR_QUEUED, CR_FLIGHT, CR_PKTS, CR_TX};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u64 x = wave_sum(s[i]);
      if (lane == 0 && x) atomicAdd(&hdr[sw[i]], (unsigned long long)x);  // (LDS)
    }
    if (lane == 0 && c_up) atomicAdd(&hdr[CR_UP], (unsigned long long)c_up);
  }
  cat_group_write(tabs, fills, ovfs, fill, ovf, p.slab + blockIdx.x);  // (its first barrier stands behind the adds above)
  if (threadIdx.x < CR_ROWS) p.part[(size_t)threadIdx.x * p.G + blockIdx.x] = (u64)hdr[threadIdx.x];
}

// workgroup g: tables 32 g .. 32 g + 31 of in[T] into out[g]
__global__ __launch_bounds__(BLOCK) void catalog_merge_kernel(const CatSlab* in, u32 T, CatSlab* out) {
  __shared__ CatTab tabs[BLOCK / 64];
  __shared__ u32 fills[BLOCK / 64], ovfs[BLOCK / 64];
  const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, per = CAT_FANIN / (BLOCK / 64);
  u32 fill = 0, ovf = 0;
  for (u32 i = 0; i < per; ++i) {
    const u32 s = blockIdx.x * CAT_FANIN + wave * per + i;  // (the same in every lane of the wave)
    if (s >= T) break;
    ovf |= in[s].ovf;
    cat_merge_from(tabs[wave], fill, ovf, lane, in[s].t, min(in[s].fill, SIM_CATALOG_LIVE));
  }
  cat_group_write(tabs, fills, ovfs, fill, ovf, out + blockIdx.x);
}

struct CatFoldP {
  const CatSlab* fin;  // the one table that is left
  const u64* part;     // [CR_ROWS][G]
  u32 G, now;          // sim_tick after the sampled tick
  u64* out;            // the sample's slot: 48 words
  u64* live;           // [SIM_CATALOG_LIVE][8]: the live table — of a running catalogue: of its latest good sample, "the previous sample" of the next
  u64* cum;            // [CS_WORDS]
  u64* reg;            // [max_ids][8]; null: sim_catalog_now, which has no registry
  u32* stamp;          // [max_ids]: 1 + the number of the good sample a record was last live in
  u32 max_ids;
};

// the place of (id, val) in a table ranked ascending, or CAT_NONE
__device__ static inline u32 cat_search(const u64* tid, const u64* tval, u32 n, u64 id, u64 val) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = (lo + hi) >> 1;
    if (cat_less(tid[mid], tval[mid], id, val)) lo = mid + 1; else hi = mid;
  }
  return lo < n && tid[lo] == id && tval[lo] == val ? lo : CAT_NONE;
}

__global__ __launch_bounds__(BLOCK) void catalog_fold_kernel(CatFoldP p) {
  enum { F_DIED = 0, F_REVIVED = 1, F_NEW = 2, F_N = 4 };
  __shared__ u64 rid[SIM_CATALOG_LIVE], rval[SIM_CATALOG_LIVE];  // the table as it came
  __shared__ CatTab s;                                            // ranked
  __shared__ u64 pid[SIM_CATALOG_LIVE], pval[SIM_CATALOG_LIVE];  // the previous good sample's identities (ranked)
  __shared__ u32 matched[SIM_CATALOG_LIVE], fresh[SIM_CATALOG_LIVE];
  __shared__ u32 cnt[F_N], kinds[3][8];
  __shared__ u64 rows[CR_ROWS];
  const u32 j = threadIdx.x;
  const bool keeps = p.reg != nullptr;
  const u32 ovf = p.fin->ovf ? 1u : 0u;
  const u32 n = ovf ? 0u : min(p.fin->fill, SIM_CATALOG_LIVE);
  const u32 reg_n = keeps ? (u32)p.cum[CS_REG] : 0u, seq = keeps ? (u32)p.cum[CS_SEQ] : 0u, prev_n = keeps ? (u32)p.cum[CS_PREV_N] : 0u;
  const u64 lost0 = keeps ? p.cum[CS_LOST] : 0ull, over0 = keeps ? p.cum[CS_OVERFLOWED] : 0ull;
  if (j < n) { rid[j] = p.fin->t.id[j]; rval[j] = p.fin->t.val[j]; }
  if (j < prev_n) { pid[j] = p.live[(size_t)j * 8]; pval[j] = p.live[(size_t)j * 8 + 1]; }
  matched[j] = 0; fresh[j] = 0;
  if (j < F_N) cnt[j] = 0;
  if (j < 24) kinds[j >> 3][j & 7u] = 0;
  for (u32 row = j >> 6; row < CR_ROWS; row += BLOCK / 64) {  // (whole waves)
    const u64 x = fold_row(p.part + (size_t)row * p.G, p.G, FOLD_SUM);
    if ((j & 63u) == 0) rows[row] = x;
  }
  __syncthreads();
  // ---- ranked by a count of smaller keys: identities are distinct, the ranks a permutation ----
  if (j < n) {
    u32 r = 0;
    for (u32 k = 0; k < n; ++k) r += cat_less(rid[k], rval[k], rid[j], rval[j]) ? 1u : 0u;
    s.id[r] = rid[j]; s.val[r] = rval[j];
#pragma unroll
    for (u32 k = 0; k < CAT_CNT; ++k) s.c[k][r] = p.fin->t.c[k][j];
  }
  __syncthreads();
  if (!ovf) {
    if (j < n) {
      const u32 kind = (u32)(s.id[j] >> 32) & 7u;
      atomicAdd(&kinds[0][kind], 1u);  // (LDS)
      atomicAdd(&kinds[1][kind], s.c[CC_QUEUED][j]);
      atomicAdd(&kinds[2][kind], s.c[CC_FLIGHT][j]);
    }
    // ---- the registry: a thread per record; records are distinct, so a place is matched by one thread at most ----
    for (u32 r = j; r < reg_n; r += BLOCK) {
      u64* rec = p.reg + (size_t)r * SIM_CATALOG_RECORD_WORDS;
      const u32 at = cat_search(s.id, s.val, n, rec[0], rec[1]);
      if (at == CAT_NONE) continue;
      matched[at] = 1;
      const bool before = seq && p.stamp[r] == seq;  // live in the previous good sample
      const u64 q = s.c[CC_QUEUED][at], hold = s.c[CC_HOLD][at];
      rec[2] = (rec[2] & 0xFFFFFFFFull) | ((u64)p.now << 32);
      rec[3] += 1ull + (before ? 0ull : 1ull << 32);
      if (q > (rec[4] & 0xFFFFFFFFull)) rec[4] = q | ((u64)p.now << 32);
      if (hold > (rec[5] & 0xFFFFFFFFull)) rec[5] = hold | ((u64)p.now << 32);
      rec[6] += s.c[CC_FLIGHT][at];
      rec[7] += q;
      p.stamp[r] = seq + 1u;
      if (!before) atomicAdd(&cnt[F_REVIVED], 1u);
    }
    if (j < prev_n && cat_search(s.id, s.val, n, pid[j], pval[j]) == CAT_NONE) atomicAdd(&cnt[F_DIED], 1u);
    __syncthreads();
    // ---- new: not in the registry, not live in the previous good sample; appended in rank order while there is room ----
    if (keeps && j < n && !matched[j] && cat_search(pid, pval, prev_n, s.id[j], s.val[j]) == CAT_NONE) fresh[j] = 1;
    __syncthreads();
    if (fresh[j]) {
      u32 pos = 0;
      for (u32 k = 0; k < j; ++k) pos += fresh[k];
      atomicAdd(&cnt[F_NEW], 1u);
      if (reg_n + pos < p.max_ids) {
        u64* rec = p.reg + (size_t)(reg_n + pos) * SIM_CATALOG_RECORD_WORDS;
        const u64 q = s.c[CC_QUEUED][j], at_now = (u64)p.now << 32;
        rec[0] = s.id[j]; rec[1] = s.val[j];
        rec[2] = (u64)p.now | at_now; rec[3] = 1ull;
        rec[4] = q | at_now; rec[5] = (u64)s.c[CC_HOLD][j] | at_now;
        rec[6] = s.c[CC_FLIGHT][j]; rec[7] = q;
        p.stamp[reg_n + pos] = seq + 1u;
      }
    }
    if (j < n) {  // (the previous table was staged before the first barrier)
      u64* e = p.live + (size_t)j * 8;
      e[0] = s.id[j]; e[1] = s.val[j]; e[2] = 0;
#pragma unroll
      for (u32 k = 0; k < CAT_CNT; ++k) e[3 + k] = s.c[k][j];
    }
  }
  __syncthreads();
  if (j == 0) {
    const u32 all_new = cnt[F_NEW], room = keeps ? p.max_ids - reg_n : 0u, added = min(all_new, room);
    u64* w = p.out;
    for (u32 k = 0; k < SIM_CATALOG_SAMPLE_WORDS; ++k) w[k] = 0;
    w[CAW_TICK] = p.now; w[CAW_UP] = rows[CR_UP];
    w[CAW_LIVE] = n; w[CAW_OVF] = ovf;
    w[CAW_QUEUED] = rows[CR_QUEUED]; w[CAW_FLIGHT] = rows[CR_FLIGHT]; w[CAW_PKTS] = rows[CR_PKTS]; w[CAW_TX] = rows[CR_TX];
    for (u32 k = 1; k < 8; ++k) {
      w[CAW_KIND_IDS + k - 1] = kinds[0][k]; w[CAW_KIND_QUEUED + k - 1] = kinds[1][k]; w[CAW_KIND_FLIGHT + k - 1] = kinds[2][k];
    }
    p.cum[CS_LIVE_N] = n;
    if (keeps) {
      w[CAW_NEW] = added; w[CAW_DIED] = cnt[F_DIED]; w[CAW_REVIVED] = cnt[F_REVIVED];
      w[CAW_REG] = reg_n + added; w[CAW_LOST] = lost0 + (all_new - added); w[CAW_OVERFLOWED] = over0 + ovf;
      p.cum[CS_REG] = reg_n + added; p.cum[CS_LOST] = w[CAW_LOST]; p.cum[CS_OVERFLOWED] = w[CAW_OVERFLOWED];
      if (!ovf) { p.cum[CS_SEQ] = seq + 1u; p.cum[CS_PREV_N] = n; }
    }
  }
}

// ---- host ----
// what a scan needs besides the sample's place
struct CatScratch {
  DevScratch<CatSlab> d_slab;  // [G], then the merge levels' [ceil(G / 32)] and [1]
  DevScratch<u64> d_part;      // [CR_ROWS][G]
  u32 G = 0;
};
static inline bool catalog_mask_ok(u32 mask) { return mask && !(mask & ~SIM_CATALOG_KINDS); }
static int catalog_prepare(const sim_handle* h, CatScratch& s) {
  s.G = (u32)std::min<size_t>(((size_t)h->d.Nl + BLOCK - 1) / BLOCK, CATALOG_GRID);
  const size_t t1 = (s.G + CAT_FANIN - 1) / CAT_FANIN;
  if (int rc = s.d_slab.alloc((size_t)s.G + t1 + 1)) return rc;
  return s.d_part.alloc((size_t)CR_ROWS * s.G);
}
// one scan of the state the stream will be in when it gets here, folded into p.out / p.live / p.cum (and the registry, when p has one)
static int catalog_launch(sim_handle* h, const CatScratch& s, u32 mask, CatFoldP p) {
  CatScanP sp;
  sp.slab = s.d_slab.get();
  sp.part = s.d_part.get();
  sp.G = s.G;
  sp.mask = mask;
  if (int rc = flight_fill(h, false, sp.fl)) return rc;
  catalog_scan_kernel<<<s.G, BLOCK, 0, h->stream>>>(h->d, sp);
  CatSlab* at = s.d_slab.get();
  for (u32 T = s.G; T > 1;) {  // 1 024 tables: 32, then 1
    const u32 T1 = (T + CAT_FANIN - 1) / CAT_FANIN;
    catalog_merge_kernel<<<T1, BLOCK, 0, h->stream>>>(at, T, at + T);
    at += T;
    T = T1;
  }
  p.fin = at;
  p.part = s.d_part.get();
  p.G = s.G;
  p.now = (u32)h->tick;
  catalog_fold_kernel<<<1, BLOCK, 0, h->stream>>>(p);
  HCHECK(hipGetLastError());
  return SIM_OK;
}
struct CatalogState : Observer {  // samples of 48 words
  CatScratch scr;
  DevScratch<u64> d_reg, d_live, d_cum;
  DevScratch<u32> d_stamp;
  u32 mask = 0, max_ids = 0;
  int setup(const sim_handle* h) {
    if (int rc = catalog_prepare(h, scr)) return rc;
    if (int rc = d_reg.alloc((size_t)max_ids * SIM_CATALOG_RECORD_WORDS)) return rc;
    if (int rc = d_stamp.alloc(max_ids)) return rc;
    if (int rc = d_live.alloc((size_t)SIM_CATALOG_LIVE * 8)) return rc;
    if (int rc = d_cum.alloc(CS_WORDS)) return rc;
    HCHECK(hipMemset(d_cum.get(), 0, CS_WORDS * 8));
    return SIM_OK;
  }
  int sample(sim_handle* h, u64* out) override {
    CatFoldP p = {};
    p.out = out; p.live = d_live.get(); p.cum = d_cum.get(); p.reg = d_reg.get(); p.stamp = d_stamp.get(); p.max_ids = max_ids;
    return catalog_launch(h, scr, mask, p);
  }
};
static inline CatalogState* catalog_of(const sim_handle* h) { return static_cast<CatalogState*>(h->obs[OB_CATALOG]); }

extern "C" {

uint32_t sim_catalog_version(void) { return SIM_CATALOG_VERSION; }

int sim_catalog_start(sim_handle* h, uint32_t kinds_mask, uint32_t max_ids, uint32_t first_tick, uint32_t period, uint32_t capacity) {
  CatalogState* s = new CatalogState();
  s->mask = kinds_mask;
  s->max_ids = max_ids;
  const auto check = [&] { return catalog_mask_ok(kinds_mask) && max_ids && max_ids <= SIM_CATALOG_MAX ? SIM_OK : SIM_EINVAL; };
  return observer_start(h, OB_CATALOG, s, SIM_CATALOG_MAX_SAMPLES, first_tick, period, capacity, SIM_CATALOG_SAMPLE_WORDS, check,
                        [&] { return s->setup(h); });
}

int sim_catalog_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_CATALOG, taken, dropped); }

int sim_catalog_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_CATALOG, first, n, out, cap_words, n_out);
}

int sim_catalog_stop(sim_handle* h) { return observer_stop(h, OB_CATALOG); }

int sim_catalog_list(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out, uint32_t* total) {
  if (int rc = observer_usable(h)) return rc;
  if (!out || !n_out || !total) return SIM_EINVAL;
  CatalogState* s = catalog_of(h);
  if (!s) return SIM_ESTATE;
  HCHECK(hipStreamSynchronize(h->stream));
  u64 cum[CS_WORDS];
  HCHECK(hipMemcpy(cum, s->d_cum.get(), sizeof cum, hipMemcpyDeviceToHost));
  const u32 have = (u32)cum[CS_REG];
  if (first > have) return SIM_EINVAL;
  const u32 got = std::min(n, have - first);
  if ((size_t)got * SIM_CATALOG_RECORD_WORDS > cap_words) return SIM_EINVAL;
  if (got) HCHECK(hipMemcpy(out, s->d_reg.get() + (size_t)first * SIM_CATALOG_RECORD_WORDS, (size_t)got * SIM_CATALOG_RECORD_WORDS * 8, hipMemcpyDeviceToHost));
  *n_out = got;
  *total = have;
  return SIM_OK;
}

int sim_catalog_live(sim_handle* h, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out || !n_out) return SIM_EINVAL;
  CatalogState* s = catalog_of(h);
  if (!s) return SIM_ESTATE;
  HCHECK(hipStreamSynchronize(h->stream));
  u64 cum[CS_WORDS];
  HCHECK(hipMemcpy(cum, s->d_cum.get(), sizeof cum, hipMemcpyDeviceToHost));
  const u32 got = (u32)cum[CS_LIVE_N];
  if ((size_t)got * 8 > cap_words) return SIM_EINVAL;
  if (got) HCHECK(hipMemcpy(out, s->d_live.get(), (size_t)got * 64, hipMemcpyDeviceToHost));
  *n_out = got;
  return SIM_OK;
}

int sim_catalog_now(sim_handle* h, uint32_t kinds_mask, uint64_t* header_out, uint64_t* live_out, size_t cap_words, uint32_t* n_out) {
  if (int rc = observer_usable(h)) return rc;
  if (!header_out || !live_out || !n_out || !catalog_mask_ok(kinds_mask)) return SIM_EINVAL;
  // scratch of its own: a running catalogue's slabs are those its samples still enqueued use; one buffer takes the sample, the count
  // and the live table
  CatScratch own;
  if (int rc = catalog_prepare(h, own)) return rc;
  const size_t words = SIM_CATALOG_SAMPLE_WORDS + CS_WORDS + (size_t)SIM_CATALOG_LIVE * 8;
  std::vector<u64> host(words);
  int rc = observer_now(h, words, host.data(), [&](u64* d_out) {
    CatFoldP p = {};
    p.out = d_out; p.cum = d_out + SIM_CATALOG_SAMPLE_WORDS; p.live = p.cum + CS_WORDS;
    return catalog_launch(h, own, kinds_mask, p);
  });
  if (rc != SIM_OK) return rc;
  const u32 got = (u32)host[SIM_CATALOG_SAMPLE_WORDS + CS_LIVE_N];
  if ((size_t)got * 8 > cap_words) return SIM_EINVAL;
  memcpy(header_out, host.data(), SIM_CATALOG_SAMPLE_WORDS * 8);
  if (got) memcpy(live_out, host.data() + SIM_CATALOG_SAMPLE_WORDS + CS_WORDS, (size_t)got * 64);
  *n_out = got;
  return SIM_OK;
}

}  // extern "C"
