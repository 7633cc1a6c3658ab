// serf_sim_detect.inc — part of the translation unit serf_sim.hip (included from there, after the ledger; not a header of its own).
// Detection log (include/serf_sim_detect.h): one kernel behind the census's count and fold, the host's bookkeeping, the entry points.
//
// Per sampled tick:
//   census_count_kernel, census_fold_kernel   (serf_sim_census.inc, through census_records) the record of every allocated slot, on scratch of
//                        the log's own: a census that runs next to it is not touched
//   detect_kernel        ONE workgroup walks the slots below the highest bound the log has seen, in chunks of BLOCK, a lane per slot: loads the
//                        slot's state (64 bytes: the open episode in the log's own format, the subject it belongs to, and three bits in the
//                        spare half of word 1) and five words of its census record, runs the state machine of the header, stores the state.
//                        A slot closes 0, 1 or 2 episodes: their places in the log are the log's length before this sample plus the closes of
//                        the chunks before (carried), of the waves before (LDS) and of the lanes before (two ballots: ">= 1", "== 2") — (sample,
//                        ascending slot) order whatever order the waves run in.  The counters and histogram bins of what closed are added up in
//                        LDS (integer adds: their order does not show) and added to the cumulative block once, by the lanes that then write the
//                        header.  No atomics on global memory.
// One workgroup: A <= 65 534 slots with a SWIM layer, 1 024 at the bench configuration — four chunks; a dense handle's N slots pay N * N entries
// in the count kernel before they get here.  Several workgroups would need the closes of all slots before theirs: a second pass, for a walk that
// the count and fold kernels outweigh by orders of magnitude.
// A handle without a started log never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_detect.h"

static_assert(sizeof(sim_detect_episode) == 64 && sizeof(sim_detect_header) == 512 && SIM_DETECT_WORDS == 64u, "layout of include/serf_sim_detect.h");

// words of a sample's header and of the cumulative block (the same places; words 0 .. 5 of the block are not used)
enum { DH_TICK = 0, DH_UP = 1, DH_SUBJECTS = 2, DH_OPEN_DOWN = 3, DH_OPEN_ACC = 4, DH_CLOSED_NOW = 5, DH_WRITTEN = 6, DH_LOST = 7, DH_OUTCOME = 8,
       DH_DECLARED = 13, DH_OPENED_DOWN = 14, DH_OPENED_ACC = 15, DH_HIST_SUSPECT = 16, DH_HIST_ALL = 32, DH_HIST_CLEARED = 48 };
// a slot's state: an episode's eight words; the high half of word 1 (0 in every record that leaves the device) holds
enum { DS_VALID = 1u, DS_PREV_RUN = 2u, DS_DONE = 4u };  // a subject is stored (word 0) / it ran at the evaluation before / `done`

struct DetDevP {
  const u64* rec;         // [bound][SIM_CENSUS_WORDS]: this tick's census records (census_records)
  const u32* subject_of;  // Dev::subject_of
  const u32* upmap;       // Dev::upmap
  u64* state;             // [A][SIM_DETECT_EPISODE_WORDS]
  u64* cum;               // [SIM_DETECT_WORDS]: the cumulative words, since the start
  u64* out;               // the sample: a header
  u64* log;               // [logcap][SIM_DETECT_EPISODE_WORDS]
  u32 N;
  u32 bound;   // slots 0 .. bound - 1 may hold a subject now (the host's high-water mark of this handle)
  u32 range;   // slots 0 .. range - 1 are evaluated: the highest bound the log has seen (>= bound; a restore can lower the handle's)
  u32 logcap;
  u32 now;     // sim_tick after the sampled tick
  u32 first;   // this is the log's first sample
};

__device__ static inline u32 detect_bin(u32 x) { return x == 0u ? 0u : min(15u, 32u - (u32)__clz((int)x)); }  // 1 + floor(log2 x)
__device__ static inline u64 pack2(u32 lo, u32 hi) { return (u64)lo | ((u64)hi << 32); }

// the episode e closes at `now` with `outcome`: its record into r, its counters and bins into the workgroup's LDS block
__device__ static inline void detect_close(const u64* e, u64* r, u32 outcome, u32 now, unsigned long long* acc) {
  const u32 w1 = (u32)e[1], kind = w1 & 0xFFu, flags = w1 >> 16, opened = (u32)e[2];
  r[0] = e[0];
  r[1] = (u64)(kind | (outcome << 8) | (flags << 16));
  r[2] = pack2(opened, now);
#pragma unroll
  for (u32 i = 3; i < SIM_DETECT_EPISODE_WORDS; ++i) r[i] = e[i];
  atomicAdd(&acc[DH_OUTCOME + outcome - 1u], 1ull);  // (LDS)
  if (kind == SIM_DETECT_ACCUSED && (u32)(e[3] >> 32) != SIM_DETECT_NEVER) atomicAdd(&acc[DH_DECLARED], 1ull);
  if (outcome == SIM_DETECT_DETECTED && !(flags & SIM_DETECT_F_CENSORED)) {
    const u32 fs = (u32)e[3], all = (u32)e[5];
    atomicAdd(&acc[DH_HIST_SUSPECT + (fs == SIM_DETECT_NEVER ? 15u : detect_bin(fs - opened))], 1ull);
    atomicAdd(&acc[DH_HIST_ALL + detect_bin(all - opened)], 1ull);
  }
  if (outcome == SIM_DETECT_CLEARED) atomicAdd(&acc[DH_HIST_CLEARED + detect_bin(now - opened)], 1ull);
}
// an episode of `kind` opens at `now` in e
__device__ static inline void detect_open(u64* e, u32 kind, u32 flags, u32 now, unsigned long long* acc) {
  const u32 nv = SIM_DETECT_NEVER;
  e[1] = (e[1] & ~0xFFFFFFFFull) | (u64)(kind | (flags << 16));
  e[2] = pack2(now, nv);
  e[3] = pack2(kind == SIM_DETECT_ACCUSED ? now : nv, nv);
  e[4] = pack2(nv, nv);
  e[5] = pack2(nv, 0u);
  e[6] = 0;
  e[7] = 0;
  atomicAdd(&acc[kind == SIM_DETECT_DOWN ? DH_OPENED_DOWN : DH_OPENED_ACC], 1ull);
}
// no episode is open in e (subject and state bits stay)
__device__ static inline void detect_none(u64* e) {
  e[1] &= ~0xFFFFFFFFull;
#pragma unroll
  for (u32 i = 2; i < SIM_DETECT_EPISODE_WORDS; ++i) e[i] = 0;
}

__global__ __launch_bounds__(BLOCK) void detect_kernel(DetDevP p) {
  __shared__ u32 wcnt[BLOCK / 64];
  __shared__ unsigned long long acc[SIM_DETECT_WORDS];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < SIM_DETECT_WORDS) acc[threadIdx.x] = 0;
  __syncthreads();
  {  // the running nodes (bits beyond N of the last word are not nodes)
    const u32 nupw = (p.N + 31u) / 32u;
    u32 c = 0;
    for (u32 w = threadIdx.x; w < nupw; w += BLOCK) {
      u32 x = p.upmap[w];
      if (w == nupw - 1u && (p.N & 31u)) x &= (1u << (p.N & 31u)) - 1u;
      c += (u32)__popc(x);
    }
    c = (u32)wave_sum(c);
    if (!lane) atomicAdd(&acc[DH_UP], (unsigned long long)c);
  }
  __syncthreads();
  const u64 R = acc[DH_UP];
  const u64 before = p.cum[DH_WRITTEN] + p.cum[DH_LOST];  // episodes closed before this sample (the block is written behind the last barrier)
  const u32 now = p.now, nv = SIM_DETECT_NEVER;
  u32 base = 0;  // episodes closed by the chunks before
  for (u32 a0 = 0; a0 < p.range; a0 += BLOCK) {  // (whole workgroups stay together: the barriers below)
    const u32 a = a0 + threadIdx.x;
    const bool inr = a < p.range;
    const u32 subj = (inr && a < p.bound) ? p.subject_of[a] : NOSLOT;
    const bool has = subj != NOSLOT;
    u64 e[SIM_DETECT_EPISODE_WORDS], r1[SIM_DETECT_EPISODE_WORDS], r2[SIM_DETECT_EPISODE_WORDS];
    u64* st = p.state + (size_t)a * SIM_DETECT_EPISODE_WORDS;
#pragma unroll
    for (u32 i = 0; i < SIM_DETECT_EPISODE_WORDS; ++i) { e[i] = inr ? st[i] : 0ull; r1[i] = 0; r2[i] = 0; }
    u32 nclosed = 0;
    const bool touched = inr && (has || ((u32)(e[1] >> 32) & DS_VALID));  // (a slot without state and without a subject: nothing to do)
    if (touched) {
      bool fresh = false;
      if (!((u32)(e[1] >> 32) & DS_VALID) || !has || (u32)e[0] != subj) {  // 1. subject change
        if ((u32)e[1] & 0xFFu) { detect_close(e, r1, SIM_DETECT_ABANDONED, now, acc); nclosed = 1; }
#pragma unroll
        for (u32 i = 0; i < SIM_DETECT_EPISODE_WORDS; ++i) e[i] = 0;
        if (has) {
          fresh = true;
          e[0] = pack2(subj, a);
          e[1] = (u64)DS_VALID << 32;
        }
      }
      if (has) {
        const u64* w = p.rec + (size_t)a * SIM_CENSUS_WORDS;
        const bool run = w[CW_UP] & 1u;
        const u64 failed = w[CW_ST + SIM_STATUS_FAILED], left = w[CW_ST + SIM_STATUS_LEFT];
        const u64 susp = w[CW_SWIM + SIM_SWIM_SUSPECT] + w[CW_SWIM + SIM_SWIM_DEAD], gone = failed + left;
        u32 sb = (u32)(e[1] >> 32), kind = (u32)e[1] & 0xFFu;
        if (run) {  // 2.
          bool returned = false;
          if (kind == SIM_DETECT_DOWN) {
            detect_close(e, nclosed ? r2 : r1, SIM_DETECT_RETURNED, now, acc);
            nclosed++;
            detect_none(e);
            kind = 0;
            returned = true;
          }
          sb &= ~DS_DONE;
          if (susp || failed) {
            if (kind != SIM_DETECT_ACCUSED) detect_open(e, SIM_DETECT_ACCUSED, returned ? SIM_DETECT_F_AFTER_RETURN : 0u, now, acc);
            if (failed && (u32)(e[3] >> 32) == nv) e[3] = pack2((u32)e[3], now);
            e[5] += 1ull << 32;  // evaluated
            e[6] = max(e[6], failed);
            e[7] = max(e[7], susp);
          } else if (kind == SIM_DETECT_ACCUSED) {
            detect_close(e, nclosed ? r2 : r1, SIM_DETECT_CLEARED, now, acc);
            nclosed++;
            detect_none(e);
          }
        } else {  // 3.
          if (kind != SIM_DETECT_DOWN && !(sb & DS_DONE) && (fresh || (sb & DS_PREV_RUN))) {
            if (kind == SIM_DETECT_ACCUSED) { detect_close(e, nclosed ? r2 : r1, SIM_DETECT_STOPPED, now, acc); nclosed++; }
            detect_open(e, SIM_DETECT_DOWN, (fresh && p.first) ? SIM_DETECT_F_CENSORED : 0u, now, acc);
            kind = SIM_DETECT_DOWN;
          }
          if (kind == SIM_DETECT_DOWN) {
            u32 fs = (u32)e[3], ff = (u32)(e[3] >> 32), half = (u32)e[4], p99 = (u32)(e[4] >> 32), all = (u32)e[5];
            if ((susp || failed) && fs == nv) fs = now;
            if (failed && ff == nv) ff = now;
            if (R) {
              if (2ull * gone >= R && half == nv) half = now;
              if (100ull * gone >= 99ull * R && p99 == nv) p99 = now;
              if (gone == R && all == nv) all = now;
            }
            e[3] = pack2(fs, ff);
            e[4] = pack2(half, p99);
            e[5] = pack2(all, (u32)(e[5] >> 32) + 1u);
            e[6] = max(e[6], gone);
            e[7] = max(e[7], susp);
            if (all != nv) {
              detect_close(e, nclosed ? r2 : r1, SIM_DETECT_DETECTED, now, acc);
              nclosed++;
              detect_none(e);
              sb |= DS_DONE;
            }
          }
        }
        sb = run ? (sb | DS_PREV_RUN) : (sb & ~DS_PREV_RUN);  // 4.
        e[1] = (e[1] & 0xFFFFFFFFull) | ((u64)sb << 32);
      }
#pragma unroll
      for (u32 i = 0; i < SIM_DETECT_EPISODE_WORDS; ++i) st[i] = e[i];
      const u32 kind = (u32)e[1] & 0xFFu;
      if (has) atomicAdd(&acc[DH_SUBJECTS], 1ull);
      if (kind) atomicAdd(&acc[kind == SIM_DETECT_DOWN ? DH_OPEN_DOWN : DH_OPEN_ACC], 1ull);
    }
    // where this lane's records go: behind those of the chunks, the waves and the lanes before it
    const u64 b1 = __ballot(nclosed >= 1u), b2 = __ballot(nclosed >= 2u);
    if (!lane) wcnt[wave] = (u32)(__popcll(b1) + __popcll(b2));
    __syncthreads();
    u32 off = base, tot = 0;
#pragma unroll
    for (u32 q = 0; q < BLOCK / 64; ++q) { off += q < wave ? wcnt[q] : 0u; tot += wcnt[q]; }
    if (nclosed) {
      const u64 below = (1ull << lane) - 1ull;
      const u64 pos = before + off + (u32)(__popcll(b1 & below) + __popcll(b2 & below));
      if (pos < p.logcap) {
        u64* dst = p.log + (size_t)pos * SIM_DETECT_EPISODE_WORDS;
#pragma unroll
        for (u32 i = 0; i < SIM_DETECT_EPISODE_WORDS; ++i) dst[i] = r1[i];
      }
      if (nclosed > 1u && pos + 1u < p.logcap) {
        u64* dst = p.log + (size_t)(pos + 1u) * SIM_DETECT_EPISODE_WORDS;
#pragma unroll
        for (u32 i = 0; i < SIM_DETECT_EPISODE_WORDS; ++i) dst[i] = r2[i];
      }
    }
    base += tot;
    __syncthreads();
  }
  if (threadIdx.x < SIM_DETECT_WORDS) {
    const u32 i = threadIdx.x;
    const u64 total = before + base;
    u64 v;
    if (i == DH_TICK) v = now;
    else if (i == DH_CLOSED_NOW) v = base;
    else if (i < DH_WRITTEN) v = acc[i];
    else {
      v = i == DH_WRITTEN ? min(total, (u64)p.logcap) : i == DH_LOST ? total - min(total, (u64)p.logcap) : p.cum[i] + acc[i];
      p.cum[i] = v;
    }
    p.out[i] = v;
  }
}

// ---- host ----
struct DetectState : Observer {  // samples of SIM_DETECT_WORDS words
  DevScratch<u64> d_part;   // [A][SIM_CENSUS_WORDS][S]: the census kernels' scratch, the log's own
  DevScratch<u64> d_rec;    // [A][SIM_CENSUS_WORDS]
  DevScratch<u64> d_state;  // [A][SIM_DETECT_EPISODE_WORDS]
  DevScratch<u64> d_cum;    // [SIM_DETECT_WORDS]
  DevScratch<u64> d_log;    // [logcap][SIM_DETECT_EPISODE_WORDS]
  u32 logcap = 0;
  u32 range = 0;  // the highest slot bound any sample has seen: the kernel's range, so that a restore to fewer slots strands no state
  int setup(sim_handle* h) {
    if (int rc = census_scratch(h, d_part, d_rec)) return rc;
    if (int rc = d_state.alloc((size_t)h->d.A * SIM_DETECT_EPISODE_WORDS)) return rc;
    if (int rc = d_cum.alloc(SIM_DETECT_WORDS)) return rc;
    if (int rc = d_log.alloc((size_t)logcap * SIM_DETECT_EPISODE_WORDS)) return rc;
    HCHECK(hipMemsetAsync(d_state.get(), 0, std::max<size_t>(h->d.A, 1) * sizeof(sim_detect_episode), h->stream));
    HCHECK(hipMemsetAsync(d_cum.get(), 0, sizeof(sim_detect_header), h->stream));
    return SIM_OK;
  }
  int sample(sim_handle* h, u64* out) override {
    const CenDevP c = census_records(h, d_part.get(), d_rec.get(), out, 0);
    DetDevP p;
    p.rec = d_rec.get(); p.subject_of = c.subject_of; p.upmap = c.upmap;
    p.state = d_state.get(); p.cum = d_cum.get(); p.out = out; p.log = d_log.get();
    p.N = c.N;
    p.bound = c.bound;
    p.range = range = std::max(range, c.bound);  // (<= A: what the state array holds)
    p.logcap = logcap;
    p.now = c.now;
    p.first = smp.taken == 0;
    detect_kernel<<<1, BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  }
};
static inline DetectState* detect_of(const sim_handle* h) { return static_cast<DetectState*>(h->obs[OB_DETECT]); }

extern "C" {

uint32_t sim_detect_version(void) { return SIM_DETECT_VERSION; }

int sim_detect_start(sim_handle* h, uint32_t first_tick, uint32_t period, uint32_t capacity, uint32_t log_capacity) {
  DetectState* s = new DetectState();
  s->logcap = log_capacity;
  return observer_start(h, OB_DETECT, s, SIM_DETECT_MAX_SAMPLES, first_tick, period, capacity, SIM_DETECT_WORDS,
                        [&] { return (log_capacity && log_capacity <= SIM_DETECT_MAX_LOG) ? SIM_OK : SIM_EINVAL; }, [&] { return s->setup(h); });
}

int sim_detect_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_DETECT, taken, dropped); }

int sim_detect_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_DETECT, first, n, out, cap_words, n_out);
}

int sim_detect_stop(sim_handle* h) { return observer_stop(h, OB_DETECT); }

int sim_detect_log_count(sim_handle* h, uint64_t* written, uint64_t* lost) {
  if (int rc = observer_usable(h)) return rc;
  if (!written || !lost) return SIM_EINVAL;
  u64 wl[2] = {0, 0};
  if (const DetectState* s = detect_of(h)) {
    HCHECK(hipStreamSynchronize(h->stream));
    HCHECK(hipMemcpy(wl, s->d_cum.get() + DH_WRITTEN, sizeof wl, hipMemcpyDeviceToHost));
  }
  *written = wl[0];
  *lost = wl[1];
  return SIM_OK;
}

int sim_detect_log_read(sim_handle* h, uint64_t first, uint32_t n, sim_detect_episode* out, uint32_t cap, uint32_t* n_out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out || !n_out) return SIM_EINVAL;
  const DetectState* s = detect_of(h);
  if (!s) return SIM_ESTATE;
  if (n > cap) return SIM_EINVAL;
  HCHECK(hipStreamSynchronize(h->stream));
  u64 written = 0;
  HCHECK(hipMemcpy(&written, s->d_cum.get() + DH_WRITTEN, sizeof written, hipMemcpyDeviceToHost));
  if (first > written || n > written - first) return SIM_EINVAL;
  if (n) HCHECK(hipMemcpy(out, s->d_log.get() + (size_t)first * SIM_DETECT_EPISODE_WORDS, (size_t)n * sizeof *out, hipMemcpyDeviceToHost));
  *n_out = n;
  return SIM_OK;
}

int sim_detect_open(sim_handle* h, sim_detect_episode* out, uint32_t cap, uint32_t* n_out) {
  if (int rc = observer_usable(h)) return rc;
  if (!n_out || (cap && !out)) return SIM_EINVAL;
  const DetectState* s = detect_of(h);
  if (!s) return SIM_ESTATE;
  HCHECK(hipStreamSynchronize(h->stream));
  std::vector<sim_detect_episode> st(s->range);  // (a copy of the state array: the open episodes are formatted here)
  if (s->range) HCHECK(hipMemcpy(st.data(), s->d_state.get(), (size_t)s->range * sizeof(sim_detect_episode), hipMemcpyDeviceToHost));
  u32 cnt = 0;
  for (const sim_detect_episode& e : st) cnt += (e.w[1] & 0xFFu) ? 1u : 0u;
  if (cnt > cap) return SIM_EINVAL;
  u32 k = 0;
  for (const sim_detect_episode& e : st) {
    if (!(e.w[1] & 0xFFu)) continue;
    out[k] = e;
    out[k++].w[1] &= 0xFFFFFFFFull;  // (the state's bits)
  }
  *n_out = cnt;
  return SIM_OK;
}

}  // extern "C"
