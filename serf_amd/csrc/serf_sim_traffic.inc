// serf_sim_traffic.inc — part of the translation unit serf_sim.hip (included from there, after the spread map; not a header of its own).
// Traffic meter (include/serf_sim_traffic.h): three kernels behind a sampled tick's last launch, the kernels of the map's reads, the host's
// bookkeeping, the entry points.
//
// Per sampled tick, in stream order:
//   traffic_send_kernel  a node per lane, grid-stride, TRAFFIC_GRID workgroups at most, whole waves kept together.  The sender walk, written
//                        out here (see the kernel): the node's map word and the third uint4 (value high bits + meta) of every page of every
//                        DISTINCT packet it sent, where they lie (obox[cur], 64- or 48-byte cells): records and units of the packet, 5 + 7
//                        bits, copied to every slot that maps to it — 16 bits a slot, a 64-bit summary a node, written as one coalesced 8-byte
//                        store (psum[Nl]).  The tx columns of the map; the header's sums through wave reductions, the record bins through LDS
//   traffic_recv_kernel  a node per lane, the same pass loop.  The packets addressed to the node (recv_packets; flight_fill puts the
//                        graph of the sampled tick in front of the stream under kRandomNodes).  Per packet ONE scattered 8-byte read of psum[sender]
//                        and the slot's 16 bits of it.  The rx columns, rx_peak, rx_down; the in-degree histogram through LDS; the two
//                        maxima travel as (value << 32) | ~id, so that one max yields the smallest id at the largest value
//   traffic_fold_kernel  one wave per word of the sample: folds its row (fold_row) into the sample's slot
// Both count kernels write their workgroup's column of ONE partial matrix [TRF_ROWS][G] as 64-bit words — no atomics on global memory,
// nothing to zero, every figure an integer, the result does not depend on order.  The map is [8][Nl] uint32_t, a plane per column: every
// access of a wave is one contiguous run.
// The reads of the map (each behind a wait for the stream — observer_settle —, on scratch of its own, the map untouched):
//   traffic_nodes_kernel  a slice of the eight planes transposed into 32-byte records
//   traffic_stat_kernel   one column: sum, max with the smallest id, min, non-zero, the histogram — ONE pass (no bin needs a figure of
//                         the pass itself, unlike the spread map's delays), its columns folded by traffic_stat_fold
//   traffic_top_kernel / traffic_top_fold   the ranking in two levels (rank_candidates / rank_merge) by (value << 32) | (0xFFFFFFFF - id):
//                         every node has a key (ALL nodes are ranked)
// A handle without a started meter never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_traffic.h"

static_assert(sizeof(sim_traffic_node) == 32 && sizeof(sim_traffic_rank) == 40 && SIM_TRAFFIC_WORDS == 64u && SIM_TRAFFIC_COLUMNS == 8u &&
              SIM_TRAFFIC_DEG_BINS == 32u && SIM_TRAFFIC_REC_BINS == 16u && SIM_TRAFFIC_SUMMARY_WORDS == 40u && SIM_TRAFFIC_BINS == 32u,
              "layout of include/serf_sim_traffic.h");
static_assert(SIM_TRAFFIC_REC_BINS == SIM_PKT_RECORDS_MAX && SIM_PKT_RECORDS_MAX < 32u && SIM_PKT_UNITS < 128u && SIM_MAX_FANOUT == 4u,
              "a slot's summary: records in 5 bits, units in 7, four slots in 64 bits");
static_assert(SIM_TRAFFIC_TOP_MAX <= BLOCK, "a workgroup has top_k candidates at most among its BLOCK nodes");

#define TRAFFIC_GRID 1024u  // workgroups of the count kernels and of the summary's pass at most
#define TRF_RANK_WORDS 5u   // a sim_traffic_rank as 64-bit words
// words of a sample and of a summary (include/serf_sim_traffic.h)
enum { TW_TICK = 0, TW_UP = 1, TW_PKTS = 2, TW_RECS = 3, TW_UNITS = 4, TW_SENDERS = 5, TW_ADDRESSED = 6, TW_DOWN = 7, TW_MAXDEG = 8,
       TW_MAXDEG_ID = 9, TW_MAXUNITS = 10, TW_MAXUNITS_ID = 11, TW_PKT_RECS = 12, TW_PKT_UNITS = 13, TW_SAMPLES = 14, TW_DEG = 16, TW_REC = 48 };
enum { TS_COLUMN = 0, TS_WIDTH = 1, TS_SUM = 2, TS_MAX = 3, TS_MAX_ID = 4, TS_MIN = 5, TS_NONZERO = 6, TS_SAMPLES = 7, TS_BIN = 8 };
// rows of the partial matrix: the send kernel's, then the receive kernel's
enum { TRS_PKTS = 0, TRS_RECS = 1, TRS_UNITS = 2, TRS_SENDERS = 3, TRS_PKT_RECS = 4, TRS_PKT_UNITS = 5, TRS_REC = 6,
       TRR_UP = TRS_REC + SIM_TRAFFIC_REC_BINS, TRR_ADDRESSED, TRR_DOWN, TRR_MAXDEG, TRR_MAXUNITS, TRR_DEG, TRF_ROWS = TRR_DEG + SIM_TRAFFIC_DEG_BINS };
// rows of the summary's pass
enum { TRT_SUM = 0, TRT_MAX = 1, TRT_MIN = 2, TRT_NONZERO = 3, TRT_BIN = 4, TRT_ROWS = TRT_BIN + SIM_TRAFFIC_BINS };

struct TrfDevP {
  u64* psum;        // [Nl]: the packets a node sent, 16 bits a slot: records | units << 5 (0: no packet)
  u32* map;         // [8][Nl]
  u64* part;        // [TRF_ROWS][G]: every workgroup of the two count kernels writes its column
  u64* out;         // the sample's slot: 64 words
  Flight fl;        // the packets of the sampled tick, its graph's rows included
  u32 G;            // workgroups of the count kernels
  u32 now;          // sim_tick after the sampled tick
  u32 samples;      // samples accumulated in the map, this one included
};

// The sender walk written out: sent_packets (serf_sim_observe.inc) with a visitor made this kernel 10 % slower on the MI355X (its slot loops
// are unrolled for the tree's per-slot registers; profiles/observer_kit.md).  A change to the walk there has to be made here as well.
__global__ __launch_bounds__(BLOCK) void traffic_send_kernel(Dev d, TrfDevP p) {
  __shared__ unsigned long long acc[TRS_REC];
  __shared__ u32 bins[SIM_TRAFFIC_REC_BINS];
  if (threadIdx.x < TRS_REC) acc[threadIdx.x] = 0;
  if (threadIdx.x < SIM_TRAFFIC_REC_BINS) bins[threadIdx.x] = 0;
  __syncthreads();
  u32 pkts = 0, recs = 0, units = 0, senders = 0, prec = 0, punits = 0;  // per lane, reduced over the wave once, at the end
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  const size_t cu4 = d.rfan ? RF_CELL_U4 : PK_U4;
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together (the reductions behind the loop need every lane)
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (l >= d.Nl) continue;
    const u32 jw = d.rfan ? d.obox[p.fl.cur][l * RF_CELL_U4 + 3u].x : d.omap[p.fl.cur][l];  // slot -> cell of the packets this node sent
    u64 sum = 0;
    u32 n_p = 0, n_r = 0, n_u = 0;
    if (jw != 0xFFFFFFFFu) {
      for (u32 k = 0; k < p.fl.nslot; ++k) {
        const u32 jb = (jw >> (8u * k)) & 0xFFu;  // first page << 2 | pages - 1
        if (jb == 0xFFu) continue;
        u32 fld = 0;
        bool again = false;
        for (u32 q = 0; q < k; ++q)
          if (((jw >> (8u * q)) & 0xFFu) == jb) { again = true; fld = (u32)(sum >> (16u * q)) & 0xFFFFu; }
        if (!again) {  // a distinct packet is read once
          u32 r_n = 0, u_n = 0;
          const u32 np = min(jb & 3u, d.PG - 1u);
          for (u32 pg = 0; pg <= np && (jb >> 2) + pg < d.fp; ++pg) {  // (never beyond the node's fp cells)
            const uint4 ch = ld4(d.obox[p.fl.cur] + ((size_t)((jb >> 2) + pg) * d.Nl + l) * cu4 + 2u);
            const u32 hw[4] = {ch.x, ch.y, ch.z, ch.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              if (!(SIM_META_KIND(hw[r]) & 7u)) continue;  // (an empty record is all zero)
              r_n++;
              u_n += 63u - ((hw[r] >> 8) & 63u);
            }
          }
          fld = r_n ? (r_n & 31u) | (min(u_n, 127u) << 5) : 0u;
        }
        if (!fld) continue;
        sum |= (u64)fld << (16u * k);
        const u32 r_n = fld & 31u, u_n = fld >> 5;
        n_p++; n_r += r_n; n_u += u_n;
        prec = max(prec, r_n); punits = max(punits, u_n);
        atomicAdd(&bins[r_n - 1u], 1u);  // (LDS; 1 <= r_n <= 16)
      }
    }
    p.psum[l] = sum;
    if (n_p) {
      p.map[(size_t)SIM_TRAFFIC_TX_PACKETS * d.Nl + l] += n_p;
      p.map[(size_t)SIM_TRAFFIC_TX_RECORDS * d.Nl + l] += n_r;
      p.map[(size_t)SIM_TRAFFIC_TX_UNITS * d.Nl + l] += n_u;
      senders++;
    }
    pkts += n_p; recs += n_r; units += n_u;
  }
  // ---- the workgroup's column ----
  lds_sum(&acc[TRS_PKTS], pkts);
  lds_sum(&acc[TRS_RECS], recs);
  lds_sum(&acc[TRS_UNITS], units);
  lds_sum(&acc[TRS_SENDERS], senders);
  lds_max(&acc[TRS_PKT_RECS], prec);
  lds_max(&acc[TRS_PKT_UNITS], punits);
  __syncthreads();
  if (threadIdx.x < TRS_REC + SIM_TRAFFIC_REC_BINS)
    p.part[(size_t)threadIdx.x * p.G + blockIdx.x] = threadIdx.x < TRS_REC ? (u64)acc[threadIdx.x] : (u64)bins[threadIdx.x - TRS_REC];
}

// ptp: the parameters of the tick that sent the packets (the bijection's map; unused under kRandomNodes)
__global__ __launch_bounds__(BLOCK) void traffic_recv_kernel(Dev d, TickP ptp, TrfDevP p) {
  __shared__ unsigned long long acc[TRR_DEG - TRR_UP];
  __shared__ u32 bins[SIM_TRAFFIC_DEG_BINS];
  if (threadIdx.x < TRR_DEG - TRR_UP) acc[threadIdx.x] = 0;
  if (threadIdx.x < SIM_TRAFFIC_DEG_BINS) bins[threadIdx.x] = 0;
  __syncthreads();
  u32 c_up = 0, c_addr = 0, c_down = 0;  // per lane, reduced over the wave once, at the end
  u64 kdeg = 0, kunits = 0;              // (value << 32) | ~id: the largest value, the smallest id among those that have it
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together (the reductions behind the loop need every lane)
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (l >= d.Nl) continue;
    u32 deg = 0, recs = 0, units = 0;
    const auto take = [&](u32 s, u32 k) {  // the packet sender s keeps for slot k: one 8-byte gather
      const u32 fld = (u32)(p.psum[s] >> (16u * k)) & 0xFFFFu;
      if (!fld) return;
      deg++; recs += fld & 31u; units += fld >> 5;
    };
    recv_packets(d, ptp, p.fl, l, take);
    const bool up = d.R1[l].z & SIM_RF_UP;
    if (deg) {
      u32* m = p.map + l;
      m[(size_t)SIM_TRAFFIC_RX_PACKETS * d.Nl] += deg;
      m[(size_t)SIM_TRAFFIC_RX_RECORDS * d.Nl] += recs;
      m[(size_t)SIM_TRAFFIC_RX_UNITS * d.Nl] += units;
      const u32 peak = m[(size_t)SIM_TRAFFIC_RX_PEAK * d.Nl];
      if (deg > peak) m[(size_t)SIM_TRAFFIC_RX_PEAK * d.Nl] = deg;
      if (!up) m[(size_t)SIM_TRAFFIC_RX_DOWN * d.Nl] += deg;
      c_addr++;
      c_down += up ? 0u : deg;
      kdeg = max(kdeg, ((u64)deg << 32) | (u64)(~(u32)l));
      kunits = max(kunits, ((u64)units << 32) | (u64)(~(u32)l));
    }
    c_up += up ? 1u : 0u;
    atomicAdd(&bins[min(deg, SIM_TRAFFIC_DEG_BINS - 1u)], 1u);  // (LDS)
  }
  // ---- the workgroup's column ----
  lds_sum(&acc[TRR_UP - TRR_UP], c_up);
  lds_sum(&acc[TRR_ADDRESSED - TRR_UP], c_addr);
  lds_sum(&acc[TRR_DOWN - TRR_UP], c_down);
  lds_max(&acc[TRR_MAXDEG - TRR_UP], kdeg);
  lds_max(&acc[TRR_MAXUNITS - TRR_UP], kunits);
  __syncthreads();
  if (threadIdx.x < TRF_ROWS - TRR_UP)
    p.part[(size_t)(TRR_UP + threadIdx.x) * p.G + blockIdx.x] =
        threadIdx.x < TRR_DEG - TRR_UP ? (u64)acc[threadIdx.x] : (u64)bins[threadIdx.x - (TRR_DEG - TRR_UP)];
}

// one wave per word of the sample; written into the sample's slot
__global__ __launch_bounds__(BLOCK) void traffic_fold_kernel(TrfDevP p) {
  const u32 w = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= SIM_TRAFFIC_WORDS) return;  // (whole waves)
  const auto row = [&](u32 r, u32 op) { return fold_row(p.part + (size_t)r * p.G, p.G, op); };
  u64 v = 0;
  if (w == TW_TICK) v = p.now;
  else if (w == TW_SAMPLES) v = p.samples;
  else if (w == TW_UP) v = row(TRR_UP, FOLD_SUM);
  else if (w >= TW_PKTS && w <= TW_SENDERS) v = row(TRS_PKTS + (w - TW_PKTS), FOLD_SUM);
  else if (w == TW_ADDRESSED) v = row(TRR_ADDRESSED, FOLD_SUM);
  else if (w == TW_DOWN) v = row(TRR_DOWN, FOLD_SUM);
  else if (w >= TW_MAXDEG && w <= TW_MAXUNITS_ID) {
    const u64 k = row(w < TW_MAXUNITS ? TRR_MAXDEG : TRR_MAXUNITS, FOLD_MAX);
    v = ((w - TW_MAXDEG) & 1u) ? ((k >> 32) ? (u64)(~(u32)k) : 0ull) : k >> 32;
  } else if (w == TW_PKT_RECS || w == TW_PKT_UNITS) v = row(TRS_PKT_RECS + (w - TW_PKT_RECS), FOLD_MAX);
  else if (w >= TW_DEG && w < TW_DEG + SIM_TRAFFIC_DEG_BINS) v = row(TRR_DEG + (w - TW_DEG), FOLD_SUM);
  else if (w >= TW_REC) v = row(TRS_REC + (w - TW_REC), FOLD_SUM);
  if (!lane) p.out[w] = v;
}

// ---- the reads of the map ----
// nodes first .. first + count - 1: the eight planes' words of a node into its 32-byte record
__global__ __launch_bounds__(BLOCK) void traffic_nodes_kernel(const u32* map, u32 Nl, u32 first, u32 count, uint4* out) {
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= count) return;
  const u32* m = map + first + i;
  out[2u * i] = make_uint4(m[0], m[(size_t)Nl], m[(size_t)2 * Nl], m[(size_t)3 * Nl]);
  out[2u * i + 1u] = make_uint4(m[(size_t)4 * Nl], m[(size_t)5 * Nl], m[(size_t)6 * Nl], m[(size_t)7 * Nl]);
}

struct TrfStatP {
  const u32* plane;  // [Nl]: the column
  u64* part;         // [TRT_ROWS][G]
  u64* out;          // the summary's 40 words
  u32 G, column, bin_width, samples;
};
__global__ __launch_bounds__(BLOCK) void traffic_stat_kernel(u32 Nl, TrfStatP p) {
  __shared__ unsigned long long acc[TRT_BIN];
  __shared__ u32 bins[SIM_TRAFFIC_BINS];
  if (threadIdx.x < TRT_BIN) acc[threadIdx.x] = threadIdx.x == TRT_MIN ? ~0ull : 0ull;
  if (threadIdx.x < SIM_TRAFFIC_BINS) bins[threadIdx.x] = 0;
  __syncthreads();
  u64 sum = 0, key = 0, lo = ~0ull;
  u32 nz = 0;
  for (size_t l = (size_t)blockIdx.x * BLOCK + threadIdx.x; l < Nl; l += (size_t)gridDim.x * BLOCK) {
    const u32 v = p.plane[l];
    sum += v;
    key = max(key, ((u64)v << 32) | (u64)(~(u32)l));
    lo = min(lo, (u64)v);
    nz += v ? 1u : 0u;
    atomicAdd(&bins[min(v / p.bin_width, SIM_TRAFFIC_BINS - 1u)], 1u);  // (LDS)
  }
  lds_sum(&acc[TRT_SUM], sum);
  lds_max(&acc[TRT_MAX], key);
  lds_sum(&acc[TRT_NONZERO], nz);
  lo = wave_min(lo);
  if ((threadIdx.x & 63) == 0) atomicMin(&acc[TRT_MIN], (unsigned long long)lo);
  __syncthreads();
  if (threadIdx.x < TRT_ROWS)
    p.part[(size_t)threadIdx.x * p.G + blockIdx.x] = threadIdx.x < TRT_BIN ? (u64)acc[threadIdx.x] : (u64)bins[threadIdx.x - TRT_BIN];
}
// one wave per word of the summary
__global__ __launch_bounds__(BLOCK) void traffic_stat_fold(TrfStatP p) {
  const u32 w = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= SIM_TRAFFIC_SUMMARY_WORDS) return;  // (whole waves)
  const auto row = [&](u32 r, u32 op) { return fold_row(p.part + (size_t)r * p.G, p.G, op); };
  u64 v;
  if (w == TS_COLUMN) v = p.column;
  else if (w == TS_WIDTH) v = p.bin_width;
  else if (w == TS_SUM) v = row(TRT_SUM, FOLD_SUM);
  else if (w == TS_MAX) v = row(TRT_MAX, FOLD_MAX) >> 32;
  else if (w == TS_MAX_ID) v = (u64)(~(u32)row(TRT_MAX, FOLD_MAX));  // (every node has a key: a cluster of zeros names node 0)
  else if (w == TS_MIN) v = row(TRT_MIN, FOLD_MIN);
  else if (w == TS_NONZERO) v = row(TRT_NONZERO, FOLD_SUM);
  else if (w == TS_SAMPLES) v = p.samples;
  else v = row(TRT_BIN + (w - TS_BIN), FOLD_SUM);
  if (!lane) p.out[w] = v;
}

struct TrfTopP {
  const u32* map;  // [8][Nl]
  u64* ckey;       // [G][top_k]: a workgroup's candidates, descending; 0 ends a shorter list
  u64* crec;       // [G][top_k][TRF_RANK_WORDS]: their records
  u64* top;        // [top_k][TRF_RANK_WORDS]
  u32 G;           // workgroups of the top kernel: ceil(Nl / BLOCK)
  u32 top_k, column;
};
__global__ __launch_bounds__(BLOCK) void traffic_top_kernel(Dev d, TrfTopP p) {
  __shared__ u64 red[2][BLOCK / 64];
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;  // the node
  const bool in = i < d.Nl;
  u32 c[SIM_TRAFFIC_COLUMNS];
#pragma unroll
  for (u32 k = 0; k < SIM_TRAFFIC_COLUMNS; ++k) c[k] = in ? p.map[(size_t)k * d.Nl + i] : 0u;
  u32 val = 0;
#pragma unroll
  for (u32 k = 0; k < SIM_TRAFFIC_COLUMNS; ++k) val = k == p.column ? c[k] : val;  // (no dynamic index into registers)
  const bool up = in && (d.R1[in ? i : 0u].z & SIM_RF_UP);
  const u64 w[TRF_RANK_WORDS] = {(u64)i | ((u64)(up ? 1u : 0u) << 32), (u64)c[0] | ((u64)c[1] << 32), (u64)c[2] | ((u64)c[3] << 32),
                                 (u64)c[4] | ((u64)c[5] << 32), (u64)c[6] | ((u64)c[7] << 32)};
  // i < 2^24: a node's key is never 0
  const u64 key = in ? ((u64)val << 32) | (u64)(0xFFFFFFFFu - i) : 0ull;
  rank_candidates<TRF_RANK_WORDS>(key, w, p.ckey, p.crec, p.top_k, red);
}
// one workgroup: the lists merged; records beyond the nodes get id 0xFFFFFFFF and zeros
__global__ __launch_bounds__(BLOCK) void traffic_top_fold(TrfTopP p) {
  __shared__ u64 red[2][BLOCK / 64];
  rank_merge<TRF_RANK_WORDS>(p.ckey, p.crec, p.G, p.top_k, p.top, red, FillNoId());
}

// ---- host ----
static inline u32 traffic_grid(const sim_handle* h) { return (u32)std::min<size_t>(((size_t)h->d.Nl + BLOCK - 1) / BLOCK, TRAFFIC_GRID); }

struct TrafficState : Observer {  // samples of 64 words
  DevScratch<u64> d_psum;  // [Nl]
  DevScratch<u32> d_map;   // [8][Nl]
  DevScratch<u64> d_part;  // [TRF_ROWS][TRAFFIC_GRID]
  // the scratch and the map (zeroed on the stream)
  int setup(sim_handle* h) {
    if (int rc = d_psum.alloc(h->d.Nl)) return rc;
    if (int rc = d_map.alloc((size_t)SIM_TRAFFIC_COLUMNS * h->d.Nl)) return rc;
    if (int rc = d_part.alloc((size_t)TRF_ROWS * TRAFFIC_GRID)) return rc;
    HCHECK(hipMemsetAsync(d_map.get(), 0, (size_t)SIM_TRAFFIC_COLUMNS * h->d.Nl * 4, h->stream));
    return SIM_OK;
  }
  int sample(sim_handle* h, u64* out) override {
    const Dev& d = h->d;
    TrfDevP p;
    p.psum = d_psum.get(); p.map = d_map.get(); p.part = d_part.get(); p.out = out;
    if (int rc = flight_fill(h, true, p.fl)) return rc;
    p.G = traffic_grid(h);
    p.now = (u32)h->tick;
    p.samples = smp.taken + 1u;
    traffic_send_kernel<<<p.G, BLOCK, 0, h->stream>>>(d, p);
    traffic_recv_kernel<<<p.G, BLOCK, 0, h->stream>>>(d, h->prev, p);
    traffic_fold_kernel<<<(SIM_TRAFFIC_WORDS + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  }
};
static inline TrafficState* traffic_of(const sim_handle* h) { return static_cast<TrafficState*>(h->obs[OB_TRAFFIC]); }

extern "C" {

uint32_t sim_traffic_version(void) { return SIM_TRAFFIC_VERSION; }

int sim_traffic_start(sim_handle* h, uint32_t first_tick, uint32_t period, uint32_t capacity) {
  TrafficState* s = new TrafficState();
  return observer_start(h, OB_TRAFFIC, s, SIM_TRAFFIC_MAX_SAMPLES, first_tick, period, capacity, SIM_TRAFFIC_WORDS, [] { return SIM_OK; },
                        [&] { return s->setup(h); });
}

int sim_traffic_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_TRAFFIC, taken, dropped); }

int sim_traffic_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_TRAFFIC, first, n, out, cap_words, n_out);
}

int sim_traffic_stop(sim_handle* h) { return observer_stop(h, OB_TRAFFIC); }

int sim_traffic_nodes(sim_handle* h, uint32_t first_node, uint32_t count, sim_traffic_node* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out || (u64)first_node + count > h->d.N) return SIM_EINVAL;
  const TrafficState* s = traffic_of(h);
  if (!s) return SIM_ESTATE;
  DevScratch<uint4> d_out;
  if (int rc = d_out.alloc((size_t)count * 2)) return rc;
  int rc = observer_settle(h, [&]() -> int {
    if (!count) return SIM_OK;
    traffic_nodes_kernel<<<(count + BLOCK - 1) / BLOCK, BLOCK, 0, h->stream>>>(s->d_map.get(), h->d.Nl, first_node, count, d_out.get());
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
  if (rc != SIM_OK) return rc;
  if (count) HCHECK(hipMemcpy(out, d_out.get(), (size_t)count * sizeof *out, hipMemcpyDeviceToHost));
  return SIM_OK;
}

int sim_traffic_top(sim_handle* h, uint32_t top_k, uint32_t column, sim_traffic_rank* top) {
  if (int rc = observer_usable(h)) return rc;
  if (!top || !top_k || top_k > SIM_TRAFFIC_TOP_MAX || column >= SIM_TRAFFIC_COLUMNS) return SIM_EINVAL;
  const TrafficState* s = traffic_of(h);
  if (!s) return SIM_ESTATE;
  return observer_read_top(h, top_k, 1u, TRF_RANK_WORDS, top, [&](u64* ckey, u64* crec, u64* d_top, u32 G) -> int {
    TrfTopP p;
    p.map = s->d_map.get(); p.ckey = ckey; p.crec = crec; p.top = d_top;
    p.G = G;
    p.top_k = top_k; p.column = column;
    traffic_top_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d, p);
    traffic_top_fold<<<1, BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
}

int sim_traffic_summary(sim_handle* h, uint32_t column, uint32_t bin_width, uint64_t* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out || !bin_width || column >= SIM_TRAFFIC_COLUMNS) return SIM_EINVAL;
  const TrafficState* s = traffic_of(h);
  if (!s) return SIM_ESTATE;
  DevScratch<u64> part, d_out;
  if (int rc = part.alloc((size_t)TRT_ROWS * traffic_grid(h))) return rc;
  if (int rc = d_out.alloc(SIM_TRAFFIC_SUMMARY_WORDS)) return rc;
  int rc = observer_settle(h, [&]() -> int {
    TrfStatP p;
    p.plane = s->d_map.get() + (size_t)column * h->d.Nl; p.part = part.get(); p.out = d_out.get();
    p.G = traffic_grid(h);
    p.column = column; p.bin_width = bin_width; p.samples = s->smp.taken;
    traffic_stat_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d.Nl, p);
    traffic_stat_fold<<<(SIM_TRAFFIC_SUMMARY_WORDS + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
  if (rc != SIM_OK) return rc;
  HCHECK(hipMemcpy(out, d_out.get(), SIM_TRAFFIC_SUMMARY_WORDS * 8, hipMemcpyDeviceToHost));
  return SIM_OK;
}

}  // extern "C"
