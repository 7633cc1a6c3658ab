// serf_sim_spread.inc — part of the translation unit serf_sim.hip (included from there, after the ledger; not a header of its own).
// Spread map (include/serf_sim_spread.h): two kernels behind a sampled tick's last launch, the kernels of the map's reads, the host's
// bookkeeping, the entry points.
//
// Per sampled tick:
//   spread_latch_kernel  a node per lane, grid-stride, SPREAD_GRID workgroups at most, whole waves kept together.  The entries —
//                        uploaded at sim_spread_start, not per sample — are staged once per workgroup in LDS (lds_stage).  Per (node, entry): one coalesced 4-byte read of the entry's plane of the map [n][Nl] and, for a running
//                        node, ONE evaluation of the shared predicate (rumour_held, serf_sim_observe.inc: view_applied / bucket_holds,
//                        slot_of and the baseline, as convergence_many_kernel uses them) — it yields `holds` and the latch alike, so the reach pass is not launched as
//                        well.  The plane is written only where a node latches.  Counts go through wave ballots and popcounts into LDS,
//                        first / last through wave_min / wave_max and an LDS min / max.  Every workgroup writes its column of a partial
//                        matrix [1 + SPR_ROWS n][G] as 64-bit words — no atomics on global memory, nothing to zero, the result does not
//                        depend on order
//   spread_fold_kernel   one wave per word of the sample: folds its row (fold_row), or — header words 3 .. 5 — the rows of every entry
// The reads of the map (each behind a wait for the stream — observer_settle —, on scratch of its own, the map untouched):
//   spread_stat_kernel / spread_hist_kernel   the summary's two passes — the bins need `first` — in the pass loop above: counts by ballots,
//                        a histogram [n][SIM_SPREAD_BINS] in LDS per workgroup, a column each; spread_scan_fold writes the words
//   spread_unreached_kernel   ONE workgroup walks the nodes in chunks of BLOCK: a node's place in the list is the unreached of the chunks
//                        before (carried), of the waves before (LDS) and of the lanes before (a ballot) — ascending id whatever order the
//                        waves run in (detect_kernel's idiom)
//   spread_late_kernel / spread_late_fold   a node per lane, a workgroup per BLOCK nodes; the record stays in the lane's registers; the
//                        ranking in two levels (rank_candidates / rank_merge) — here with the two-word key (score + 1, 0xFFFFFFFF - id):
//                        missed, late_sum and the id together need more than 64 bits
// A handle without a started map never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_spread.h"

static_assert(sizeof(sim_spread_entry) == 16 && sizeof(sim_spread_node) == 64 && SIM_SPREAD_MAX == SIM_CONV_MAX && SIM_SPREAD_MAX == 64u &&
              SIM_SPREAD_HEADER_WORDS == 8u && SIM_SPREAD_ENTRY_WORDS == 8u && SIM_SPREAD_SUMMARY_WORDS == 40u && SIM_SPREAD_BINS == 32u,
              "layout of include/serf_sim_spread.h");
static_assert(SIM_SPREAD_TOP_MAX <= BLOCK, "a workgroup has top_k candidates at most among its BLOCK nodes");

#define SPREAD_GRID 1024u  // workgroups of the latch kernel and of the summary's passes at most
#define SPR_ROWS 6u        // rows of the partial matrix an entry: words SE_NEW .. SE_LAST
#define SPR_STAT 5u        // rows an entry of the summary's first pass: first, last, reached, reached_up, unreached_up
#define SPR_HIST (1u + SIM_SPREAD_BINS)  // of its second: the sum of the delays, the bins
// words of the header, of an entry, of an entry's summary and of a node's record (include/serf_sim_spread.h)
enum { SH_TICK = 0, SH_UP = 1, SH_N = 2, SH_NEW = 3, SH_STARTED = 4, SH_FULL = 5 };
enum { SE_ID = 0, SE_VAL = 1, SE_NEW = 2, SE_REACHED = 3, SE_REACHED_UP = 4, SE_HOLDS = 5, SE_FIRST = 6, SE_LAST = 7 };
enum { SS_ID = 0, SS_VAL = 1, SS_FIRST = 2, SS_LAST = 3, SS_REACHED = 4, SS_REACHED_UP = 5, SS_UNREACHED_UP = 6, SS_LATE = 7, SS_BIN = 8 };
enum { SN_ID = 0, SN_GOT = 1, SN_MISSED = 2, SN_LATE_SUM = 3, SN_LATE_MAX = 4 };

// the entries as the kernels read them: built and uploaded once, at sim_spread_start
struct SprTab {
  u64 id[SIM_SPREAD_MAX];     // key | kind << 32
  u64 ltime[SIM_SPREAD_MAX];
  u32 n, pad;
};

struct SprDevP {
  const SprTab* tab;
  u32* map;    // [n][Nl]: arrival, 0 = not yet
  u64* part;   // [1 + SPR_ROWS n][G]: every workgroup of the latch kernel writes its column
  u64* out;    // the sample's slot: 8 + 8 n words
  u32 G;       // workgroups of the latch kernel
  u32 n;       // entries
  u32 now;     // sim_tick after the sampled tick
};

__global__ __launch_bounds__(BLOCK) void spread_latch_kernel(Dev d, const uint4* base, SprDevP p) {
  __shared__ SprTab tab;
  __shared__ u32 cnt[SIM_SPREAD_MAX * 4];  // new, reached, reached_up, holds
  __shared__ u32 lo[SIM_SPREAD_MAX], hi[SIM_SPREAD_MAX];
  __shared__ u32 s_up;
  lds_stage(tab, p.tab);
  for (u32 i = threadIdx.x; i < SIM_SPREAD_MAX * 4; i += BLOCK) cnt[i] = 0;
  if (threadIdx.x < SIM_SPREAD_MAX) { lo[threadIdx.x] = 0xFFFFFFFFu; hi[threadIdx.x] = 0; }
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
    for (u32 e = 0; e < p.n; ++e) {
      u32* cell = p.map + (size_t)e * d.Nl + l;
      u32 a = in ? *cell : 0u;
      const u64 id = tab.id[e];
      const bool hit = up && rumour_held(d, base, l, (u32)(id >> 32), (u32)id, tab.ltime[e]);
      const bool latch = hit && a == 0u;
      if (latch) { *cell = p.now; a = p.now; }
      const u64 mn = __ballot(latch), mr = __ballot(a != 0u), mru = __ballot(a != 0u && up), mh = __ballot(hit);
      if (mr | mh) {  // (the same in every lane)
        const u32 vmin = (u32)wave_min(a ? (u64)a : 0xFFFFFFFFull), vmax = (u32)wave_max((u64)a);
        if (lane0) {
          if (mn) atomicAdd(&cnt[e * 4 + 0], (u32)__popcll(mn));
          if (mr) { atomicAdd(&cnt[e * 4 + 1], (u32)__popcll(mr)); atomicMin(&lo[e], vmin); atomicMax(&hi[e], vmax); }
          if (mru) atomicAdd(&cnt[e * 4 + 2], (u32)__popcll(mru));
          if (mh) atomicAdd(&cnt[e * 4 + 3], (u32)__popcll(mh));
        }
      }
    }
  }
  __syncthreads();
  // ---- the workgroup's column: row 0 the running nodes, then SPR_ROWS rows an entry ----
  for (u32 w = threadIdx.x; w < 1u + SPR_ROWS * p.n; w += BLOCK) {
    u64 v;
    if (w == 0) v = s_up;
    else {
      const u32 e = (w - 1u) / SPR_ROWS, c = (w - 1u) % SPR_ROWS;
      v = c < 4u ? (u64)cnt[e * 4 + c] : c == 4u ? (lo[e] == 0xFFFFFFFFu ? ~0ull : (u64)lo[e]) : (u64)hi[e];
    }
    p.part[(size_t)w * p.G + blockIdx.x] = v;
  }
}

// one wave per word of the sample; written into the sample's slot
__global__ __launch_bounds__(BLOCK) void spread_fold_kernel(SprDevP p) {
  const u32 w = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= SIM_SPREAD_HEADER_WORDS + SIM_SPREAD_ENTRY_WORDS * p.n) return;  // (whole waves)
  const auto row = [&](u32 e, u32 word) { return p.part + (size_t)(1u + e * SPR_ROWS + (word - SE_NEW)) * p.G; };
  u64 v = 0;
  if (w < SIM_SPREAD_HEADER_WORDS) {
    if (w == SH_TICK) v = p.now;
    else if (w == SH_N) v = p.n;
    else if (w == SH_UP) v = fold_row(p.part, p.G, FOLD_SUM);
    else if (w == SH_NEW) { for (u32 e = 0; e < p.n; ++e) v += fold_row(row(e, SE_NEW), p.G, FOLD_SUM); }
    else if (w == SH_STARTED) { for (u32 e = 0; e < p.n; ++e) v += fold_row(row(e, SE_REACHED), p.G, FOLD_SUM) ? 1u : 0u; }
    else if (w == SH_FULL) {
      const u64 up = fold_row(p.part, p.G, FOLD_SUM);
      for (u32 e = 0; e < p.n; ++e) v += (up && fold_row(row(e, SE_REACHED_UP), p.G, FOLD_SUM) == up) ? 1u : 0u;
    }
  } else {
    const u32 i = (w - SIM_SPREAD_HEADER_WORDS) / SIM_SPREAD_ENTRY_WORDS, c = (w - SIM_SPREAD_HEADER_WORDS) % SIM_SPREAD_ENTRY_WORDS;
    if (c == SE_ID) v = p.tab->id[i];
    else if (c == SE_VAL) v = p.tab->ltime[i];
    else if (c == SE_FIRST) { v = fold_row(row(i, c), p.G, FOLD_MIN); v = v == ~0ull ? 0ull : v; }
    else v = fold_row(row(i, c), p.G, c == SE_LAST ? FOLD_MAX : FOLD_SUM);
  }
  if (!lane) p.out[w] = v;
}

// ---- the reads of the map ----
struct SprScanP {
  const SprTab* tab;
  const u32* map;  // [n][Nl]
  u64* part;       // first pass [SPR_STAT n][G], second pass [SPR_HIST n][G]
  u64* out;        // [n][stride]: an entry's summary, words SS_ID ..
  u32 G, n;
  u32 stride;      // words an entry of out: SIM_SPREAD_SUMMARY_WORDS, or 8 when only the first pass runs (sim_spread_late)
  u32 bin_width;
  u32 pass;        // what spread_scan_fold folds: 0 the first pass, 1 the second
};

// the summary's first pass: per entry first, last, reached, reached_up, unreached_up
__global__ __launch_bounds__(BLOCK) void spread_stat_kernel(Dev d, SprScanP p) {
  __shared__ u32 cnt[SIM_SPREAD_MAX * 3];  // reached, reached_up, unreached_up
  __shared__ u32 lo[SIM_SPREAD_MAX], hi[SIM_SPREAD_MAX];
  for (u32 i = threadIdx.x; i < SIM_SPREAD_MAX * 3; i += BLOCK) cnt[i] = 0;
  if (threadIdx.x < SIM_SPREAD_MAX) { lo[threadIdx.x] = 0xFFFFFFFFu; hi[threadIdx.x] = 0; }
  __syncthreads();
  const bool lane0 = (threadIdx.x & 63) == 0;
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together: the ballots below need every lane
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in = l < d.Nl;
    const bool up = in && (d.R1[l].z & SIM_RF_UP);
    for (u32 e = 0; e < p.n; ++e) {
      const u32 a = in ? p.map[(size_t)e * d.Nl + l] : 0u;
      const u64 mr = __ballot(a != 0u), mru = __ballot(a != 0u && up), mun = __ballot(a == 0u && up);
      if (mr) {  // (the same in every lane)
        const u32 vmin = (u32)wave_min(a ? (u64)a : 0xFFFFFFFFull), vmax = (u32)wave_max((u64)a);
        if (lane0) { atomicAdd(&cnt[e * 3 + 0], (u32)__popcll(mr)); atomicMin(&lo[e], vmin); atomicMax(&hi[e], vmax); }  // (LDS)
      }
      if (lane0 && mru) atomicAdd(&cnt[e * 3 + 1], (u32)__popcll(mru));
      if (lane0 && mun) atomicAdd(&cnt[e * 3 + 2], (u32)__popcll(mun));
    }
  }
  __syncthreads();
  for (u32 w = threadIdx.x; w < SPR_STAT * p.n; w += BLOCK) {
    const u32 e = w / SPR_STAT, c = w % SPR_STAT;
    p.part[(size_t)w * p.G + blockIdx.x] = c == 0u ? (lo[e] == 0xFFFFFFFFu ? ~0ull : (u64)lo[e]) : c == 1u ? (u64)hi[e] : (u64)cnt[e * 3 + (c - 2u)];
  }
}

// the summary's second pass, behind the first pass's fold: per entry the sum of arrival - first and the delays' histogram
__global__ __launch_bounds__(BLOCK) void spread_hist_kernel(Dev d, SprScanP p) {
  __shared__ u32 first[SIM_SPREAD_MAX];
  __shared__ u32 bins[SIM_SPREAD_MAX * SIM_SPREAD_BINS];
  __shared__ unsigned long long late[SIM_SPREAD_MAX];
  for (u32 i = threadIdx.x; i < SIM_SPREAD_MAX * SIM_SPREAD_BINS; i += BLOCK) bins[i] = 0;
  if (threadIdx.x < SIM_SPREAD_MAX) {
    first[threadIdx.x] = threadIdx.x < p.n ? (u32)p.out[(size_t)threadIdx.x * p.stride + SS_FIRST] : 0u;
    late[threadIdx.x] = 0;
  }
  __syncthreads();
  const bool lane0 = (threadIdx.x & 63) == 0;
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together: the wave's sum below needs every lane
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in = l < d.Nl;
    for (u32 e = 0; e < p.n; ++e) {
      if (!first[e]) continue;  // (nobody has an arrival; the same in every lane)
      const u32 a = in ? p.map[(size_t)e * d.Nl + l] : 0u;
      const u32 delay = a ? a - first[e] : 0u;
      if (a) atomicAdd(&bins[e * SIM_SPREAD_BINS + min(delay / p.bin_width, SIM_SPREAD_BINS - 1u)], 1u);  // (LDS)
      const u64 s = wave_sum((u64)delay);
      if (lane0 && s) atomicAdd(&late[e], (unsigned long long)s);
    }
  }
  __syncthreads();
  for (u32 w = threadIdx.x; w < SPR_HIST * p.n; w += BLOCK) {
    const u32 e = w / SPR_HIST, c = w % SPR_HIST;
    p.part[(size_t)w * p.G + blockIdx.x] = c == 0u ? (u64)late[e] : (u64)bins[e * SIM_SPREAD_BINS + (c - 1u)];
  }
}

// one wave per word a pass yields: pass 0 words SS_ID .. SS_UNREACHED_UP of every entry, pass 1 words SS_LATE ..
__global__ __launch_bounds__(BLOCK) void spread_scan_fold(SprScanP p) {
  const u32 w = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const u32 per = p.pass ? SPR_HIST : SS_LATE;
  if (w >= per * p.n) return;  // (whole waves)
  const u32 e = w / per, c = w % per;
  u64 v;
  if (p.pass) v = fold_row(p.part + (size_t)(e * SPR_HIST + c) * p.G, p.G, FOLD_SUM);
  else if (c == SS_ID) v = p.tab->id[e];
  else if (c == SS_VAL) v = p.tab->ltime[e];
  else {
    v = fold_row(p.part + (size_t)(e * SPR_STAT + (c - SS_FIRST)) * p.G, p.G, c == SS_FIRST ? FOLD_MIN : c == SS_LAST ? FOLD_MAX : FOLD_SUM);
    if (c == SS_FIRST && v == ~0ull) v = 0;
  }
  if (!lane) p.out[(size_t)e * p.stride + (p.pass ? SS_LATE : 0u) + c] = v;
}

// the running nodes with arrival 0 of one plane, ascending: ids[0 .. min(cap, total) - 1], *total
__global__ __launch_bounds__(BLOCK) void spread_unreached_kernel(Dev d, const u32* plane, u32* ids, u32 cap, u32* total) {
  __shared__ u32 wcnt[BLOCK / 64];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u32 base = 0;  // the unreached of the chunks before
  for (size_t l0 = 0; l0 < d.Nl; l0 += BLOCK) {  // (whole workgroups stay together: the barriers below)
    const size_t l = l0 + threadIdx.x;
    const bool un = l < d.Nl && (d.R1[l].z & SIM_RF_UP) && plane[l] == 0u;
    const u64 bal = __ballot(un);
    if (!lane) wcnt[wave] = (u32)__popcll(bal);
    __syncthreads();
    u32 off = base, tot = 0;
#pragma unroll
    for (u32 q = 0; q < BLOCK / 64; ++q) { off += q < wave ? wcnt[q] : 0u; tot += wcnt[q]; }
    if (un) {
      const u32 pos = off + (u32)__popcll(bal & ((1ull << lane) - 1ull));
      if (pos < cap) ids[pos] = (u32)l;
    }
    base += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = base;
}

struct SprLateP {
  const u32* map;   // [n][Nl]
  const u64* stat;  // [n][8]: the first pass's words (SS_FIRST is read)
  u64* ckey;        // [G][top_k][2]: a workgroup's candidates, descending: (score + 1, 0xFFFFFFFF - id); a first half of 0 ends a shorter list
  u64* crec;        // [G][top_k][SIM_SPREAD_NODE_WORDS]: their records
  u64* nodes;       // null, or [Nl][SIM_SPREAD_NODE_WORDS]
  u64* top;         // [top_k][SIM_SPREAD_NODE_WORDS]
  u32 G;            // workgroups of the late kernel: ceil(Nl / BLOCK)
  u32 n, top_k, rank_by;
};
__global__ __launch_bounds__(BLOCK) void spread_late_kernel(Dev d, SprLateP p) {
  __shared__ u32 first[SIM_SPREAD_MAX];
  __shared__ WideKey red[2][BLOCK / 64];
  if (threadIdx.x < SIM_SPREAD_MAX) first[threadIdx.x] = threadIdx.x < p.n ? (u32)p.stat[(size_t)threadIdx.x * 8u + SS_FIRST] : 0u;
  __syncthreads();
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;  // the node
  const bool in = i < d.Nl;
  const bool up = in && (d.R1[in ? i : 0u].z & SIM_RF_UP);
  u32 got = 0, missed = 0, late_max = 0;
  u64 late_sum = 0;
  for (u32 e = 0; e < p.n; ++e) {
    const u32 f = first[e];
    if (!f || !in) continue;  // (an entry nobody has an arrival for is not started)
    const u32 a = p.map[(size_t)e * d.Nl + i];
    if (a) { got++; late_sum += a - f; late_max = max(late_max, a - f); }
    else missed++;
  }
  u64 w[SIM_SPREAD_NODE_WORDS] = {(u64)i | ((u64)(up ? 1u : 0u) << 32), got, missed, late_sum, late_max, 0, 0, 0};
  if (p.nodes && in) {
    u64* dst = p.nodes + (size_t)i * SIM_SPREAD_NODE_WORDS;
#pragma unroll
    for (u32 k = 0; k < SIM_SPREAD_NODE_WORDS; ++k) dst[k] = w[k];
  }
  // the key: unique among the running nodes.  late_sum < 64 * 2^32, missed <= 64
  WideKey key = {0, 0};
  if (up) {
    key.s = 1ull + (p.rank_by == SIM_SPREAD_BY_MISSED ? ((u64)missed << 40) | late_sum : (late_sum << 8) | (u64)missed);
    key.r = (u64)(0xFFFFFFFFu - i);
  }
  rank_candidates<SIM_SPREAD_NODE_WORDS>(key, w, p.ckey, p.crec, p.top_k, red);
}

// one workgroup: the lists merged; writes the listed records, zeroing what stays unused
__global__ __launch_bounds__(BLOCK) void spread_late_fold(SprLateP p) {
  __shared__ WideKey red[2][BLOCK / 64];
  rank_merge<SIM_SPREAD_NODE_WORDS>(p.ckey, p.crec, p.G, p.top_k, p.top, red, FillZero());
}

// ---- host ----
static inline size_t spread_stride(u32 n) { return SIM_SPREAD_HEADER_WORDS + (size_t)n * SIM_SPREAD_ENTRY_WORDS; }  // words of a sample
static inline u32 spread_grid(const sim_handle* h) { return (u32)std::min<size_t>(((size_t)h->d.Nl + BLOCK - 1) / BLOCK, SPREAD_GRID); }

// the entries checked and put into the kernels' form; touches nothing but t
static int spread_check(const sim_handle* h, const sim_spread_entry* e, u32 n, SprTab& t) {
  if (!e || !n || n > SIM_SPREAD_MAX) return SIM_EINVAL;
  memset(&t, 0, sizeof t);
  t.n = n;
  for (u32 i = 0; i < n; ++i) {
    const u32 kind = e[i].kind, key = e[i].key;
    if (kind < SIM_K_JOIN || kind > SIM_K_QUERY) return SIM_EINVAL;
    const bool named = kind == SIM_K_EVENT || kind == SIM_K_QUERY;  // the key is a name, not a subject
    if (named ? key == 0 : key >= h->d.N) return SIM_EINVAL;
    if (e[i].ltime >> 48) return SIM_EINVAL;
    for (u32 j = 0; j < i; ++j)
      if (e[j].kind == kind && e[j].key == key && e[j].ltime == e[i].ltime) return SIM_EINVAL;
    t.id[i] = (u64)key | ((u64)kind << 32);
    t.ltime[i] = e[i].ltime;
  }
  return SIM_OK;
}

struct SpreadState : Observer {  // samples of 8 + 8 n words
  DevScratch<SprTab> d_tab;
  DevScratch<u32> d_map;    // [n][Nl]
  DevScratch<u64> d_part;   // [1 + SPR_ROWS n][SPREAD_GRID]
  u32 n = 0;
  // checks, then the ring planes the predicate reads (the route sim_track_add takes), the map (zeroed on the stream) and the table's upload
  int setup(sim_handle* h, const sim_spread_entry* e, u32 cnt) {
    SprTab t;
    if (int rc = spread_check(h, e, cnt, t)) return rc;
    for (u32 i = 0; i < cnt; ++i)
      if (int rc = conv_plane(h, e[i].kind, e[i].ltime)) return rc;
    n = cnt;
    if (int rc = d_tab.alloc(1)) return rc;
    if (int rc = d_map.alloc((size_t)n * h->d.Nl)) return rc;
    if (int rc = d_part.alloc((1u + (size_t)SPR_ROWS * n) * SPREAD_GRID)) return rc;
    HCHECK(hipMemcpy(d_tab.get(), &t, sizeof t, hipMemcpyHostToDevice));
    HCHECK(hipMemsetAsync(d_map.get(), 0, (size_t)n * h->d.Nl * 4, h->stream));
    return SIM_OK;
  }
  int sample(sim_handle* h, u64* out) override {
    SprDevP p;
    p.tab = d_tab.get(); p.map = d_map.get(); p.part = d_part.get(); p.out = out;
    p.G = spread_grid(h);
    p.n = n;
    p.now = (u32)h->tick;
    spread_latch_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d, h->d_base, p);
    const u32 words = (u32)spread_stride(n);
    spread_fold_kernel<<<(words + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  }
};
static inline SpreadState* spread_of(const sim_handle* h) { return static_cast<SpreadState*>(h->obs[OB_SPREAD]); }

// the summary's first pass and its fold into out[n][stride] (the stream's order puts both behind the samples enqueued so far)
static int spread_stat_launch(sim_handle* h, const SpreadState* s, SprScanP& p, u64* part, u64* out, u32 stride) {
  p.tab = s->d_tab.get(); p.map = s->d_map.get(); p.part = part; p.out = out;
  p.G = spread_grid(h);
  p.n = s->n;
  p.stride = stride;
  p.bin_width = 1;
  p.pass = 0;
  spread_stat_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d, p);
  spread_scan_fold<<<(SS_LATE * p.n + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
  HCHECK(hipGetLastError());
  return SIM_OK;
}

extern "C" {

uint32_t sim_spread_version(void) { return SIM_SPREAD_VERSION; }

int sim_spread_start(sim_handle* h, const sim_spread_entry* e, uint32_t n, uint32_t first_tick, uint32_t period, uint32_t capacity) {
  SpreadState* s = new SpreadState();
  const auto check = [&] {
    SprTab t;
    return spread_check(h, e, n, t);
  };
  return observer_start(h, OB_SPREAD, s, SIM_SPREAD_MAX_SAMPLES, first_tick, period, capacity, spread_stride(n), check,
                        [&] { return s->setup(h, e, n); });
}

int sim_spread_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_SPREAD, taken, dropped); }

int sim_spread_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_SPREAD, first, n, out, cap_words, n_out);
}

int sim_spread_stop(sim_handle* h) { return observer_stop(h, OB_SPREAD); }

int sim_spread_map(sim_handle* h, uint32_t entry, uint32_t first_node, uint32_t count, uint32_t* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out) return SIM_EINVAL;
  const SpreadState* s = spread_of(h);
  if (!s) return SIM_ESTATE;
  if (entry >= s->n || (u64)first_node + count > h->d.N) return SIM_EINVAL;
  HCHECK(hipStreamSynchronize(h->stream));
  if (count) HCHECK(hipMemcpy(out, s->d_map.get() + (size_t)entry * h->d.Nl + first_node, (size_t)count * 4, hipMemcpyDeviceToHost));
  return SIM_OK;
}

int sim_spread_summary(sim_handle* h, uint32_t bin_width, uint64_t* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out || !bin_width) return SIM_EINVAL;
  const SpreadState* s = spread_of(h);
  if (!s) return SIM_ESTATE;
  const size_t G = spread_grid(h), words = (size_t)s->n * SIM_SPREAD_SUMMARY_WORDS;
  DevScratch<u64> part, d_out;
  if (int rc = part.alloc((size_t)SPR_HIST * s->n * G)) return rc;  // (SPR_HIST >= SPR_STAT: both passes' columns fit)
  if (int rc = d_out.alloc(words)) return rc;
  int rc = observer_settle(h, [&]() -> int {
    SprScanP p;
    if (int lrc = spread_stat_launch(h, s, p, part.get(), d_out.get(), SIM_SPREAD_SUMMARY_WORDS)) return lrc;
    p.bin_width = bin_width;
    p.pass = 1;
    spread_hist_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d, p);
    spread_scan_fold<<<(SPR_HIST * p.n + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
  if (rc != SIM_OK) return rc;
  HCHECK(hipMemcpy(out, d_out.get(), words * 8, hipMemcpyDeviceToHost));
  return SIM_OK;
}

int sim_spread_unreached(sim_handle* h, uint32_t entry, uint32_t* ids, uint32_t cap, uint32_t* n_out, uint32_t* total) {
  if (int rc = observer_usable(h)) return rc;
  if (!n_out || !total || (cap && !ids)) return SIM_EINVAL;
  const SpreadState* s = spread_of(h);
  if (!s) return SIM_ESTATE;
  if (entry >= s->n) return SIM_EINVAL;
  return observer_read_ids(h, ids, cap, n_out, total, [&](u32* d_ids, u32 room, u32* d_total) -> int {
    spread_unreached_kernel<<<1, BLOCK, 0, h->stream>>>(h->d, s->d_map.get() + (size_t)entry * h->d.Nl, d_ids, room, d_total);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
}

int sim_spread_late(sim_handle* h, uint32_t top_k, uint32_t rank_by, sim_spread_node* top, sim_spread_node* nodes) {
  if (int rc = observer_usable(h)) return rc;
  if (!top || !top_k || top_k > SIM_SPREAD_TOP_MAX || rank_by > SIM_SPREAD_BY_LATE) return SIM_EINVAL;
  const SpreadState* s = spread_of(h);
  if (!s) return SIM_ESTATE;
  DevScratch<u64> part, d_stat, d_nodes;
  if (int rc = part.alloc((size_t)SPR_STAT * s->n * spread_grid(h))) return rc;
  if (int rc = d_stat.alloc((size_t)s->n * 8)) return rc;
  if (nodes)
    if (int rc = d_nodes.alloc((size_t)h->d.Nl * SIM_SPREAD_NODE_WORDS)) return rc;
  int rc = observer_read_top(h, top_k, 2u, SIM_SPREAD_NODE_WORDS, top, [&](u64* ckey, u64* crec, u64* d_top, u32 G) -> int {
    SprScanP sp;
    if (int lrc = spread_stat_launch(h, s, sp, part.get(), d_stat.get(), 8)) return lrc;
    SprLateP p;
    p.map = s->d_map.get(); p.stat = d_stat.get(); p.ckey = ckey; p.crec = crec;
    p.nodes = nodes ? d_nodes.get() : nullptr;
    p.top = d_top;
    p.G = G;
    p.n = s->n; p.top_k = top_k; p.rank_by = rank_by;
    spread_late_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d, p);
    spread_late_fold<<<1, BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
  if (rc != SIM_OK) return rc;
  if (nodes) HCHECK(hipMemcpy(nodes, d_nodes.get(), (size_t)h->d.N * sizeof *nodes, hipMemcpyDeviceToHost));
  return SIM_OK;
}

}  // extern "C"
