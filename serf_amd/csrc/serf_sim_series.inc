// serf_sim_series.inc — part of the translation unit serf_sim.hip (included from there, after the trackers; not a header of its own).
// Device-resident time series (include/serf_sim_series.h): two kernels behind a sampled tick's last launch, the host's bookkeeping, the entry points.
//
// Per sampled tick:
//   series_sample_kernel  a node per lane, grid-stride; reads the row groups, the queue's sort keys the node's count says are in use and
//                         the packets where their senders keep them; histogram bins by ballot into wave-uniform counters, sums / mins /
//                         maxes by wave reduction, one column of a partial matrix [64 words][workgroups] per workgroup — integers
//                         throughout, no atomics on global memory, nothing to zero
//   series_fold_kernel    one wave per word: adds its row up (or takes its min / max), writes the word into the sample's slot
// Their order is the stream's.  The host knows every sampled tick in advance: it passes the slot to the launch and reads nothing back.
// A handle without a started series never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_series.h"

static_assert(sizeof(sim_series_sample) == 512 && SIM_SERIES_WORDS == 64u, "layout of include/serf_sim_series.h");

#define SER_GRID 1024u  // workgroups of the sample kernel at most
// words of a sample (include/serf_sim_series.h)
enum {
  SW_TICK = 0, SW_UP = 1, SW_STATE = 2, SW_QCLS = 6, SW_BIN = 10, SW_MAXDEPTH = 18, SW_AW = 19, SW_TIMERS = 27, SW_TNODES = 28,
  SW_FAILED = 29, SW_LEFT = 30, SW_KMIN = 31, SW_KMAX = 32, SW_CLK = 33, SW_OVERFLOW = 39, SW_PKTS = 40, SW_KIND = 41, SW_LEN = 48,
  SW_USED = 49
};
// how a word's partial results combine
__host__ __device__ static inline u32 ser_op(u32 w) {
  if (w == SW_KMIN || w == SW_CLK || w == SW_CLK + 2 || w == SW_CLK + 4) return FOLD_MIN;
  if (w == SW_MAXDEPTH || w == SW_KMAX || w == SW_CLK + 1 || w == SW_CLK + 3 || w == SW_CLK + 5) return FOLD_MAX;
  return FOLD_SUM;
}

struct SerDevP {
  u64* part;   // [SIM_SERIES_WORDS][G]: every workgroup of the sample kernel writes its column
  u64* out;    // the sample's slot of the device buffer: SIM_SERIES_WORDS words
  u32 G;       // workgroups of the sample kernel
  u32 now;     // sim_tick after the sampled tick
  u32 cur;     // parity of the cells that hold the packets in flight (obox[cur] / omap[cur])
  u32 nslot;   // fan-out slots that carry packets: f (random fan-out), feff of the tick that sent them (bijection)
};

__global__ __launch_bounds__(BLOCK) void series_sample_kernel(Dev d, SerDevP p) {
  __shared__ u64 acc[SIM_SERIES_WORDS];
  if (threadIdx.x < SIM_SERIES_WORDS) acc[threadIdx.x] = ser_op(threadIdx.x) == FOLD_MIN ? ~0ull : 0ull;
  __syncthreads();
  // counts of nodes: a ballot per bin, kept per wave (the same value in every lane: scalar registers)
  u32 c_up = 0, c_tn = 0, c_state[4] = {0, 0, 0, 0}, c_bin[8] = {0, 0, 0, 0, 0, 0, 0, 0}, c_aw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // sums, mins and maxes: per lane, reduced over the wave once, at the end
  u32 qc[4] = {0, 0, 0, 0}, timers = 0, pkts = 0, len = 0, mxd = 0, kmin = 0xFFFFFFFFu, kmax = 0;
  u64 nfail = 0, nleft = 0, ovf = 0, kinds_lo = 0, kinds_hi = 0;  // kinds: 16-bit fields, kind & 3 of each half
  u64 cmin[3] = {~0ull, ~0ull, ~0ull}, cmax[3] = {0, 0, 0};
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  const size_t cu4 = d.rfan ? RF_CELL_U4 : PK_U4;
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together: the ballots below need every lane
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in = l < d.Nl;
    uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0, r2 = r0, r3 = r0;
    u32 jw = 0xFFFFFFFFu;
    if (in) {
      r0 = ld4(&d.R0[l]); r1 = ld4(&d.R1[l]); r2 = ld4(&d.R2[l]); r3 = ld4(&d.R3[l]);
      jw = d.rfan ? d.obox[p.cur][l * RF_CELL_U4 + 3u].x : d.omap[p.cur][l];  // slot -> cell of the packets this node sent
    }
    const bool up = in && (r1.z & SIM_RF_UP);
    ovf += r2.w;  // (every node: the model-bound counter)
    // ---- the node's row ----
    u32 cnt = 0, bin = 0, ntim = 0;
    if (up) {
      cnt = q_count(d, l, r2.z);
      bin = cnt ? 32u - (u32)__clz((int)cnt) : 0u;
      mxd = max(mxd, cnt);
      nfail += r2.x; nleft += r2.y;
      kmin = min(kmin, r1.w); kmax = max(kmax, r1.w);
      const u64 ck[3] = {(u64)r0.x | ((u64)r0.y << 32), (u64)r0.z | ((u64)r0.w << 32), (u64)r1.x | ((u64)r1.y << 32)};
#pragma unroll
      for (int i = 0; i < 3; ++i) { cmin[i] = ck[i] < cmin[i] ? ck[i] : cmin[i]; cmax[i] = ck[i] > cmax[i] ? ck[i] : cmax[i]; }
      // the queue: keys ascending, the class their top bits — a class's entries are the positions between two boundaries
      u32 lt1 = 0, lt2 = 0, lt3 = 0;
      for (u32 g = 0; 4u * g < cnt; ++g) {
        const uint4 k = ld4(&d.qkeys[(size_t)g * d.Nl + l]);
        const u32 kk[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
          const bool v = 4u * g + j < cnt;
          lt1 += (v && kk[j] < (1u << QK_CLS_SH)) ? 1u : 0u;
          lt2 += (v && kk[j] < (2u << QK_CLS_SH)) ? 1u : 0u;
          lt3 += (v && kk[j] < (3u << QK_CLS_SH)) ? 1u : 0u;
        }
      }
      qc[0] += lt1; qc[1] += lt2 - lt1; qc[2] += lt3 - lt2; qc[3] += cnt - lt3;
      if (r3.y) {  // susp_next: a node without a deadline runs no timer
        const uint4 ta = ld4(&d.R4[2 * l]), tb = ld4(&d.R4[2 * l + 1]);
        const u32 tw[8] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) ntim += ((tw[i] & 0xFFFFu) ? 1u : 0u) + ((tw[i] >> 16) ? 1u : 0u);
        timers += ntim;
      }
    }
    c_up += (u32)__popcll(__ballot(up));
    c_tn += (u32)__popcll(__ballot(ntim != 0));
    const u32 st = SIM_RF_STATE(r1.z);
#pragma unroll
    for (u32 i = 0; i < 4; ++i) c_state[i] += (u32)__popcll(__ballot(up && st == i));
#pragma unroll
    for (u32 i = 0; i < 8; ++i) {
      c_bin[i] += (u32)__popcll(__ballot(up && bin == i));
      c_aw[i] += (u32)__popcll(__ballot(up && r3.z == i));
    }
    // ---- the packets this node sent last tick, where they lie: a distinct packet weighs as many slots as map to it ----
    if (jw != 0xFFFFFFFFu) {
      for (u32 k = 0; k < p.nslot; ++k) {
        const u32 jb = (jw >> (8u * k)) & 0xFFu;  // first page << 2 | pages - 1
        if (jb == 0xFFu) continue;
        bool again = false;
        u32 wgt = 0;
        for (u32 q = 0; q < p.nslot; ++q) {
          const bool same = ((jw >> (8u * q)) & 0xFFu) == jb;
          again |= same && q < k;
          wgt += same ? 1u : 0u;
        }
        if (again) continue;
        u32 any = 0;
        const u32 np = min(jb & 3u, d.PG - 1u);
        for (u32 pg = 0; pg <= np && (jb >> 2) + pg < d.fp; ++pg) {  // (never beyond the node's fp cells)
          const uint4 ch = ld4(d.obox[p.cur] + ((size_t)((jb >> 2) + pg) * d.Nl + l) * cu4 + 2u);
          const u32 hw[4] = {ch.x, ch.y, ch.z, ch.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const u32 kind = SIM_META_KIND(hw[r]) & 7u;
            if (!kind) continue;  // (an empty record is all zero)
            any = 1;
            const u64 one = (u64)wgt << (16u * (kind & 3u));
            if (kind & 4u) kinds_hi += one; else kinds_lo += one;
            len += wgt * (63u - ((hw[r] >> 8) & 63u));
          }
        }
        pkts += any ? wgt : 0u;
      }
    }
  }
  // ---- the workgroup's column ----
  const bool lane0 = (threadIdx.x & 63) == 0;
  if (lane0) {
    atomicAdd((unsigned long long*)&acc[SW_UP], (unsigned long long)c_up);
    atomicAdd((unsigned long long*)&acc[SW_TNODES], (unsigned long long)c_tn);
#pragma unroll
    for (u32 i = 0; i < 4; ++i) atomicAdd((unsigned long long*)&acc[SW_STATE + i], (unsigned long long)c_state[i]);
#pragma unroll
    for (u32 i = 0; i < 8; ++i) {
      atomicAdd((unsigned long long*)&acc[SW_BIN + i], (unsigned long long)c_bin[i]);
      atomicAdd((unsigned long long*)&acc[SW_AW + i], (unsigned long long)c_aw[i]);
    }
  }
  // (the kinds: 16-bit fields per lane, spread out to 32 bits of room before they are added up over the wave)
  const u64 s[14] = {qc[0], qc[1], qc[2], qc[3], timers, nfail, nleft, ovf, pkts, len,
                     ((kinds_lo >> 16) & 0xFFFFull) | (((kinds_lo >> 48) & 0xFFFFull) << 32),   // kinds 1, 3
                     ((kinds_lo >> 32) & 0xFFFFull) | ((kinds_hi & 0xFFFFull) << 32),            // kinds 2, 4
                     ((kinds_hi >> 16) & 0xFFFFull) | (((kinds_hi >> 48) & 0xFFFFull) << 32),   // kinds 5, 7
                     (kinds_hi >> 32) & 0xFFFFull};                                              // kind 6
  const u32 sw[14] = {SW_QCLS, SW_QCLS + 1, SW_QCLS + 2, SW_QCLS + 3, SW_TIMERS, SW_FAILED, SW_LEFT, SW_OVERFLOW, SW_PKTS, SW_LEN,
                      SW_KIND + 0, SW_KIND + 1, SW_KIND + 4, SW_KIND + 5};
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    const u64 v = wave_sum(s[i]);
    if (!lane0 || !v) continue;
    if (i < 10) atomicAdd((unsigned long long*)&acc[sw[i]], (unsigned long long)v);
    else {  // two kinds in one word: the second is two kinds further on
      atomicAdd((unsigned long long*)&acc[sw[i]], (unsigned long long)(v & 0xFFFFFFFFull));
      if (v >> 32) atomicAdd((unsigned long long*)&acc[sw[i] + 2], (unsigned long long)(v >> 32));
    }
  }
  {
    const u64 vmin[4] = {kmin == 0xFFFFFFFFu ? ~0ull : (u64)kmin, cmin[0], cmin[1], cmin[2]};
    const u64 vmax[5] = {kmax, cmax[0], cmax[1], cmax[2], mxd};
    const u32 wmin[4] = {SW_KMIN, SW_CLK, SW_CLK + 2, SW_CLK + 4}, wmax[5] = {SW_KMAX, SW_CLK + 1, SW_CLK + 3, SW_CLK + 5, SW_MAXDEPTH};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u64 v = wave_min(vmin[i]);
      if (lane0) atomicMin((unsigned long long*)&acc[wmin[i]], (unsigned long long)v);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const u64 v = wave_max(vmax[i]);
      if (lane0) atomicMax((unsigned long long*)&acc[wmax[i]], (unsigned long long)v);
    }
  }
  __syncthreads();
  if (threadIdx.x < SIM_SERIES_WORDS) p.part[(size_t)threadIdx.x * p.G + blockIdx.x] = acc[threadIdx.x];
}

// one wave per word of the sample: its row of the partial matrix added up (or its min / max taken), written into the sample's slot
__global__ __launch_bounds__(BLOCK) void series_fold_kernel(SerDevP p) {
  const u32 w = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= SIM_SERIES_WORDS) return;  // (whole waves)
  u64 v = w == SW_TICK ? (u64)p.now : 0ull;
  if (w != SW_TICK && w < SW_USED) {
    v = fold_row(p.part + (size_t)w * p.G, p.G, ser_op(w));
    if (ser_op(w) == FOLD_MIN && v == ~0ull) v = 0;  // no node runs
  }
  if (!lane) p.out[w] = v;
}

// ---- host ----
struct SeriesState : Observer {  // samples of SIM_SERIES_WORDS words
  DevScratch<u64> d_part;  // [SIM_SERIES_WORDS][SER_GRID]
  int sample(sim_handle* h, u64* out) override {
    const Dev& d = h->d;
    SerDevP p;
    p.part = d_part.get();
    p.out = out;
    p.G = (u32)std::min<size_t>(((size_t)d.Nl + BLOCK - 1) / BLOCK, SER_GRID);
    p.now = (u32)h->tick;
    p.cur = (u32)(h->tick & 1);
    p.nslot = d.rfan ? d.f : h->prev.feff;  // (h->prev: the parameters of the tick that just ended, the one that sent the packets)
    series_sample_kernel<<<p.G, BLOCK, 0, h->stream>>>(d, p);
    series_fold_kernel<<<SIM_SERIES_WORDS / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  }
};

extern "C" {

uint32_t sim_series_version(void) { return SIM_SERIES_VERSION; }

int sim_series_start(sim_handle* h, uint32_t first_tick, uint32_t period, uint32_t capacity) {
  SeriesState* s = new SeriesState();
  return observer_start(h, OB_SERIES, s, SIM_SERIES_MAX_SAMPLES, first_tick, period, capacity, SIM_SERIES_WORDS,
                        [] { return SIM_OK; }, [&] { return s->d_part.alloc((size_t)SIM_SERIES_WORDS * SER_GRID); });
}

int sim_series_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_SERIES, taken, dropped); }

int sim_series_read(sim_handle* h, uint32_t first, uint32_t n, sim_series_sample* out, uint32_t* n_out) {
  return observer_read(h, OB_SERIES, first, n, out, ~(size_t)0, n_out);
}

int sim_series_stop(sim_handle* h) { return observer_stop(h, OB_SERIES); }

}  // extern "C"
