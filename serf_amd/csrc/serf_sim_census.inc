// serf_sim_census.inc — part of the translation unit serf_sim.hip (included from there, after the series; not a header of its own).
// Membership census (include/serf_sim_census.h): three kernels behind a sampled tick's last launch, the host's bookkeeping, the entry points.
//
// Per sampled tick:
//   census_count_kernel  a workgroup per (view slot, segment of CEN_SEG nodes); leaves at once when subject_of[slot] is no node — decided
//                        on the device: slots are handed out and given back while sim_step(h, n) runs ahead, the launch knows only the
//                        host's high-water mark.  Lanes stride over the segment's nodes, ONE 16-byte head load per entry (the tail plane is
//                        never touched, a free slot's plane — which may have no memory — never read); whether the observer runs is a bit
//                        of d.upmap (ops_kernel keeps it current; a handle that holds every node has shard0 == 0, so local index == node id,
//                        vshards or not), staged once per workgroup in LDS: 1 bit per entry, not a second row load.  The ten counts are
//                        6-bit fields of one 64-bit register per lane, the four extremes a register (pair) each; one wave reduction at the
//                        end, one partial record per (slot, segment) — integers throughout, no atomics on global memory, nothing to zero
//   census_fold_kernel   a wave per slot: adds the segments' partial records up (or takes their min / max), looks the subject's own
//                        liveness up in d.upmap, writes the record into a scratch array [slots]
//   census_pack_kernel   workgroup 0 walks the slots in ascending order, compacts the allocated ones into the sample (the first
//                        max_subjects of them) and computes the header over ALL of them; the other workgroups zero the records that stay unused
// Their order is the stream's.  The host knows every sampled tick in advance: it passes the sample's place to the launches and reads nothing back.
// A handle without a started census never gets here (sim_step_end finds its entry of the observers' table null).
//
// The segment.  CEN_SEG = 8192 nodes = 128 KiB of heads per workgroup of 256 lanes: 32 loads a lane, issued in batches of CEN_BATCH = 8
// independent ones (128 bytes a lane, 32 KiB a workgroup in flight — with 8 workgroups a CU about what the latency-bandwidth product of
// HBM asks of a CU).  At 1 Mi nodes a slot is 128 segments: 64 allocated slots are 8 192 workgroups, 32 per CU of the 256 — several
// rounds, so the tail of the last round is a few per cent — while a workgroup's closing reduction (about 100 cross-lane steps) stays an
// eighth of its 32 x ~25 instructions of counting.  A lane counts at most 32 entries per field: a 6-bit field holds it.
#include "../../include/serf_sim_census.h"

static_assert(sizeof(sim_census_subject) == 128 && sizeof(sim_census_header) == 128 && SIM_CENSUS_WORDS == 16u, "layout of include/serf_sim_census.h");

#define CEN_SEG 8192u
#define CEN_BATCH 8u
#define CEN_ZREC 64u  // records a zeroing workgroup of the pack kernel covers
static_assert(CEN_SEG / 32u == BLOCK, "a lane stages one word of the liveness bitmap");
static_assert(CEN_SEG / BLOCK < 64u && (CEN_SEG / BLOCK) % CEN_BATCH == 0u, "a lane's count of one bin is a 6-bit field");
static_assert(SIM_STATUS_FAILED == 4, "five status bins");
// words of a subject's record (include/serf_sim_census.h); a partial record has words CW_ST .. CW_INCMAX
enum { CW_ID = 0, CW_UP = 1, CW_ST = 2, CW_SWIM = 7, CW_INTENT = 11, CW_LTMIN = 12, CW_LTMAX = 13, CW_INCMIN = 14, CW_INCMAX = 15 };
enum { CH_TICK = 0, CH_UP = 1, CH_SUBJECTS = 2, CH_STORED = 3, CH_SETTLED = 4, CH_FF_SUBJ = 5, CH_FF_PAIRS = 6, CH_SUSP_SUBJ = 7,
       CH_SUSP_PAIRS = 8, CH_UNDET_SUBJ = 9, CH_UNDET_PAIRS = 10, CH_DETECTED = 11 };

struct CenDevP {
  const uint4* view;      // Dev::view: the head planes, [A][Nl]
  const u32* subject_of;  // Dev::subject_of
  const u32* upmap;       // Dev::upmap
  u32 N, Nl;
  u64* part;   // [bound][SIM_CENSUS_WORDS][S]: the partial record of every (slot, segment), word-major so that the fold reads rows
  u64* rec;    // [bound][SIM_CENSUS_WORDS]: the record of every allocated slot
  u64* out;    // the sample: a header, then maxsub records
  u32 S;       // segments a slot has: ceil(Nl / CEN_SEG)
  u32 bound;   // slots 0 .. bound - 1 are looked at (the host's high-water mark; which of them are allocated the device decides)
  u32 maxsub;  // records a sample holds
  u32 now;     // sim_tick after the sampled tick
};

__global__ __launch_bounds__(BLOCK) void census_count_kernel(CenDevP p) {
  const u32 a = blockIdx.x / p.S, seg = blockIdx.x - a * p.S;
  if (p.subject_of[a] == NOSLOT) return;  // (the same in every lane; a free slot's plane is not read)
  __shared__ u32 upw[CEN_SEG / 32u];
  __shared__ u64 red[BLOCK / 64][8];
  const u32 l0 = seg * CEN_SEG, nseg = min(CEN_SEG, p.Nl - l0), nupw = (p.N + 31u) / 32u;
  {
    const u32 wi = (l0 >> 5) + threadIdx.x;
    upw[threadIdx.x] = wi < nupw ? p.upmap[wi] : 0u;
  }
  __syncthreads();
  const uint4* plane = p.view + (size_t)a * p.Nl + l0;
  u64 cnt = 0, ltmin = ~0ull, ltmax = 0;
  u32 imin = 0xFFFFFFFFu, imax = 0;
  const u32 ubit = threadIdx.x & 31u, uword = threadIdx.x >> 5;  // (l0 is a multiple of 32: the bit of node l0 + i is bit i & 31 of word i >> 5)
#pragma unroll 1
  for (u32 it0 = 0; it0 < CEN_SEG / BLOCK; it0 += CEN_BATCH) {  // (one batch of loads in flight a lane: 8 x 4 registers)
    uint4 e[CEN_BATCH];
#pragma unroll
    for (u32 j = 0; j < CEN_BATCH; ++j) {
      const u32 i = (it0 + j) * BLOCK + threadIdx.x;
      e[j] = ld4(&plane[min(i, nseg - 1u)]);  // (beyond the segment's end: its last entry once more, not counted — the batch's loads stay unconditional)
    }
#pragma unroll
    for (u32 j = 0; j < CEN_BATCH; ++j) {
      const u32 i = (it0 + j) * BLOCK + threadIdx.x;
      const bool up = i < nseg && ((upw[(it0 + j) * (BLOCK / 32u) + uword] >> ubit) & 1u);
      const u32 bits = e[j].w;
      const bool known = up && (bits & SIM_VB_KNOWN);
      const u32 st = known ? SIM_VB_STATUS(bits) : SIM_STATUS_NONE;
      u64 add = 1ull << (6u * min(st, (u32)SIM_STATUS_FAILED));
      add |= known ? 1ull << (30u + 6u * SIM_VB_SWIM(bits)) : (SIM_VB_INTENT(bits) ? 1ull << 54 : 0ull);
      cnt += up ? add : 0ull;
      const u64 lt = (u64)e[j].x | ((u64)e[j].y << 32);
      ltmin = (known && lt < ltmin) ? lt : ltmin;
      ltmax = (known && lt > ltmax) ? lt : ltmax;
      imin = known ? min(imin, e[j].z) : imin;
      imax = known ? max(imax, e[j].z) : imax;
    }
  }
  // the lane's ten 6-bit fields, spread to 16 bits of room each (a wave's sum is at most 64 * 32), then one reduction over the wave
  u64 s[3] = {0, 0, 0};
#pragma unroll
  for (u32 k = 0; k < 10; ++k) s[k >> 2] |= ((cnt >> (6u * k)) & 63ull) << (16u * (k & 3u));
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = wave_sum(s[k]);
  ltmin = wave_min(ltmin); ltmax = wave_max(ltmax);
  const u64 ilo = wave_min((u64)imin), ihi = wave_max((u64)imax);
  if ((threadIdx.x & 63) == 0) {
    u64* r = red[threadIdx.x >> 6];
    r[0] = s[0]; r[1] = s[1]; r[2] = s[2]; r[3] = ltmin; r[4] = ltmax; r[5] = ilo; r[6] = ihi;
  }
  __syncthreads();
  if (threadIdx.x < 14u) {  // word CW_ST + threadIdx.x of the partial record
    const u32 w = threadIdx.x;
    u64 v;
    if (w < 10u) {
      v = 0;
      for (u32 q = 0; q < BLOCK / 64; ++q) v += (red[q][w >> 2] >> (16u * (w & 3u))) & 0xFFFFull;
    } else {
      const bool mn = w == 10u || w == 12u;
      v = mn ? ~0ull : 0ull;
      for (u32 q = 0; q < BLOCK / 64; ++q) {
        const u64 y = red[q][w - 7u];
        v = mn ? (y < v ? y : v) : (y > v ? y : v);
      }
    }
    p.part[((size_t)a * SIM_CENSUS_WORDS + CW_ST + w) * p.S + seg] = v;
  }
}

// a wave per slot: the segments' partial records combined, the subject's own liveness, the record into rec[slot]
__global__ __launch_bounds__(BLOCK) void census_fold_kernel(CenDevP p) {
  const u32 a = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= p.bound) return;  // (whole waves)
  const u32 subj = p.subject_of[a];
  if (subj == NOSLOT) return;  // (the pack kernel asks subject_of too: rec[a] is not read)
  // (fourteen rows in ONE pass, their loads in flight together: fold_row fourteen times is fourteen loops — six more VGPRs, a wave less per SIMD)
  u64 v[14];
#pragma unroll
  for (u32 w = 0; w < 14; ++w) v[w] = (w == 10u || w == 12u) ? ~0ull : 0ull;
  const u64* row = p.part + ((size_t)a * SIM_CENSUS_WORDS + CW_ST) * p.S;
  for (u32 g = lane; g < p.S; g += 64) {
#pragma unroll
    for (u32 w = 0; w < 14; ++w) {
      const u64 y = row[(size_t)w * p.S + g];
      v[w] = w < 10u ? v[w] + y : (w == 10u || w == 12u) ? (y < v[w] ? y : v[w]) : (y > v[w] ? y : v[w]);
    }
  }
#pragma unroll
  for (u32 w = 0; w < 14; ++w) v[w] = w < 10u ? wave_sum(v[w]) : (w == 10u || w == 12u) ? wave_min(v[w]) : wave_max(v[w]);
  if (lane) return;
  u64* r = p.rec + (size_t)a * SIM_CENSUS_WORDS;
  const bool anyknown = (v[5] | v[6] | v[7] | v[8]) != 0;  // (the swim bins: the known observers)
  r[CW_ID] = (u64)subj | ((u64)a << 32);
  r[CW_UP] = (p.upmap[subj >> 5] >> (subj & 31u)) & 1u;
#pragma unroll
  for (u32 w = 0; w < 10; ++w) r[CW_ST + w] = v[w];
#pragma unroll
  for (u32 w = 10; w < 14; ++w) r[CW_ST + w] = anyknown ? v[w] : 0ull;
}

// the sample: workgroup 0 compacts the allocated slots' records in ascending slot order and computes the header over all of them;
// workgroup b > 0 zeroes what stays unused of records (b - 1) * CEN_ZREC .. b * CEN_ZREC - 1
__global__ __launch_bounds__(BLOCK) void census_pack_kernel(CenDevP p) {
  __shared__ u32 wcnt[BLOCK / 64];
  __shared__ unsigned long long hacc[SIM_CENSUS_WORDS];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x > 0) {
    // how many subjects there are: every zeroing workgroup counts for itself (bound words of subject_of, out of the L2)
    if (threadIdx.x == 0) hacc[0] = 0;
    __syncthreads();
    u32 c = 0;
    for (u32 a = threadIdx.x; a < p.bound; a += BLOCK) c += p.subject_of[a] != NOSLOT ? 1u : 0u;
    c = (u32)wave_sum(c);
    if (!lane) atomicAdd(&hacc[0], (unsigned long long)c);  // (LDS)
    __syncthreads();
    const u32 stored = (u32)min((u64)hacc[0], (u64)p.maxsub);
    const u32 r0 = (blockIdx.x - 1u) * CEN_ZREC, r1 = min(r0 + CEN_ZREC, p.maxsub);
    const u32 z0 = max(r0, stored);
    if (z0 >= r1) return;
    u64* o = p.out + (size_t)(1u + z0) * SIM_CENSUS_WORDS;
    for (u32 i = threadIdx.x; i < (r1 - z0) * SIM_CENSUS_WORDS; i += BLOCK) o[i] = 0;
    return;
  }
  if (threadIdx.x < SIM_CENSUS_WORDS) hacc[threadIdx.x] = 0;
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
    if (!lane) atomicAdd(&hacc[CH_UP], (unsigned long long)c);
  }
  __syncthreads();
  const u64 R = hacc[CH_UP];
  u32 base = 0;
  u32 hs[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // header words 4 .. 11, this lane's share (counts of subjects and of (observer, subject) pairs: below 2^32 ... per lane)
  u64 hp[3] = {0, 0, 0};                   // the pair sums (words 6, 8, 10)
  for (u32 a0 = 0; a0 < p.bound; a0 += BLOCK) {  // (whole workgroups stay together: the barriers below)
    const u32 a = a0 + threadIdx.x;
    const bool valid = a < p.bound && p.subject_of[a] != NOSLOT;
    const u64 bal = __ballot(valid);
    if (!lane) wcnt[wave] = (u32)__popcll(bal);
    __syncthreads();
    u32 off = base, tot = 0;
#pragma unroll
    for (u32 q = 0; q < BLOCK / 64; ++q) { off += q < wave ? wcnt[q] : 0u; tot += wcnt[q]; }
    if (valid) {
      const u32 r = off + (u32)__popcll(bal & ((1ull << lane) - 1ull));
      const u64* src = p.rec + (size_t)a * SIM_CENSUS_WORDS;
      u64 w[SIM_CENSUS_WORDS];
#pragma unroll
      for (u32 i = 0; i < SIM_CENSUS_WORDS; ++i) w[i] = src[i];
      if (r < p.maxsub) {
        u64* dst = p.out + (size_t)(1u + r) * SIM_CENSUS_WORDS;
#pragma unroll
        for (u32 i = 0; i < SIM_CENSUS_WORDS; ++i) dst[i] = w[i];
      }
      if (R) {
        bool one_st = false, one_sw = false;
#pragma unroll
        for (u32 i = 1; i < 5; ++i) one_st |= w[CW_ST + i] == R;
#pragma unroll
        for (u32 i = 0; i < 4; ++i) one_sw |= w[CW_SWIM + i] == R;
        const bool settled = w[CW_ST] == R || (one_st && one_sw && w[CW_LTMIN] == w[CW_LTMAX] && w[CW_INCMIN] == w[CW_INCMAX]);
        const bool run = w[CW_UP] & 1u;
        const u64 failed = w[CW_ST + SIM_STATUS_FAILED], susp = w[CW_SWIM + SIM_SWIM_SUSPECT] + w[CW_SWIM + SIM_SWIM_DEAD];
        const u64 alive = w[CW_ST + SIM_STATUS_ALIVE], gone = failed + w[CW_ST + SIM_STATUS_LEFT];
        hs[0] += settled ? 1u : 0u;
        hs[1] += (run && failed) ? 1u : 0u;   hp[0] += run ? failed : 0ull;
        hs[3] += (run && susp) ? 1u : 0u;     hp[1] += run ? susp : 0ull;
        hs[5] += (!run && alive) ? 1u : 0u;   hp[2] += !run ? alive : 0ull;
        hs[7] += (!run && gone == R) ? 1u : 0u;
      }
    }
    base += tot;
    __syncthreads();
  }
  {
    const u64 v[8] = {hs[0], hs[1], hp[0], hs[3], hp[1], hs[5], hp[2], hs[7]};
#pragma unroll
    for (u32 i = 0; i < 8; ++i) {
      const u64 t = wave_sum(v[i]);
      if (!lane && t) atomicAdd(&hacc[CH_SETTLED + i], (unsigned long long)t);
    }
  }
  if (threadIdx.x == 0) {
    hacc[CH_TICK] = p.now;
    hacc[CH_SUBJECTS] = base;
    hacc[CH_STORED] = min(base, p.maxsub);
  }
  __syncthreads();
  if (threadIdx.x < SIM_CENSUS_WORDS) p.out[threadIdx.x] = hacc[threadIdx.x];
}

// ---- host ----
static inline u32 census_segments(const sim_handle* h) { return (h->d.Nl + CEN_SEG - 1u) / CEN_SEG; }
static inline size_t census_stride(u32 maxsub) { return ((size_t)maxsub + 1u) * SIM_CENSUS_WORDS; }  // words of a sample

// the kernels' scratch, for every slot the handle can ever hand out
static int census_scratch(const sim_handle* h, DevScratch<u64>& part, DevScratch<u64>& rec) {
  const u64 cells = (u64)h->d.A * census_segments(h);
  if (cells > 0x7FFFFFFFull) return SIM_ENOMEM;  // (a grid of that many workgroups; its partial records alone would be 256 GiB)
  if (int rc = part.alloc((size_t)cells * SIM_CENSUS_WORDS)) return rc;
  return rec.alloc((size_t)h->d.A * SIM_CENSUS_WORDS);
}
// the record of every allocated slot into rec (the count and fold kernels; the roll runs them too); returns the parameters they got
static CenDevP census_records(sim_handle* h, u64* part, u64* rec, u64* out, u32 maxsub) {
  CenDevP p;
  p.view = h->d.view; p.subject_of = h->d.subject_of; p.upmap = h->d.upmap;
  p.N = h->d.N; p.Nl = h->d.Nl;
  p.part = part; p.rec = rec; p.out = out;
  p.S = census_segments(h);
  p.bound = std::min(h->n_slots, h->d.A);  // the host hands the slots out itself, in the stream's order: none beyond its high-water mark is in use
  p.maxsub = maxsub;
  p.now = (u32)h->tick;
  if (p.bound) {
    census_count_kernel<<<p.bound * p.S, BLOCK, 0, h->stream>>>(p);
    census_fold_kernel<<<(p.bound + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
  }
  return p;
}
// one census of the state the stream will be in when it gets here, into out[(1 + maxsub) * SIM_CENSUS_WORDS]
static int census_launch(sim_handle* h, u64* part, u64* rec, u64* out, u32 maxsub) {
  const CenDevP p = census_records(h, part, rec, out, maxsub);
  census_pack_kernel<<<1u + (maxsub + CEN_ZREC - 1u) / CEN_ZREC, BLOCK, 0, h->stream>>>(p);
  HCHECK(hipGetLastError());
  return SIM_OK;
}
struct CensusState : Observer {  // samples of (1 + maxsub) * SIM_CENSUS_WORDS words
  DevScratch<u64> d_part;  // [A][SIM_CENSUS_WORDS][S]
  DevScratch<u64> d_rec;   // [A][SIM_CENSUS_WORDS]
  u32 maxsub = 0;
  int sample(sim_handle* h, u64* out) override { return census_launch(h, d_part.get(), d_rec.get(), out, maxsub); }
};

extern "C" {

uint32_t sim_census_version(void) { return SIM_CENSUS_VERSION; }

int sim_census_start(sim_handle* h, uint32_t first_tick, uint32_t period, uint32_t capacity, uint32_t max_subjects) {
  CensusState* s = new CensusState();
  s->maxsub = max_subjects;
  return observer_start(h, OB_CENSUS, s, SIM_CENSUS_MAX_SAMPLES, first_tick, period, capacity, census_stride(max_subjects),
                        [&] { return max_subjects ? SIM_OK : SIM_EINVAL; }, [&] { return census_scratch(h, s->d_part, s->d_rec); });
}

int sim_census_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_CENSUS, taken, dropped); }

int sim_census_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_CENSUS, first, n, out, cap_words, n_out);
}

int sim_census_stop(sim_handle* h) { return observer_stop(h, OB_CENSUS); }

int sim_census_now(sim_handle* h, sim_census_header* hdr, sim_census_subject* recs, uint32_t cap, uint32_t* n) {
  if (int rc = observer_usable(h)) return rc;
  if (!hdr || !n || (cap && !recs)) return SIM_EINVAL;
  const u32 maxsub = std::min(cap, h->d.A);  // (there are no more subjects than slots)
  DevScratch<u64> own_part, own_rec;
  // (a running census lends its scratch: the stream orders the two uses)
  CensusState* run = static_cast<CensusState*>(h->obs[OB_CENSUS]);
  if (!run) { if (int rc = census_scratch(h, own_part, own_rec)) return rc; }
  u64* part = run ? run->d_part.get() : own_part.get();
  u64* rec = run ? run->d_rec.get() : own_rec.get();
  std::vector<u64> host(census_stride(maxsub));
  if (int rc = observer_now(h, host.size(), host.data(), [&](u64* out) { return census_launch(h, part, rec, out, maxsub); })) return rc;
  memcpy(hdr, host.data(), sizeof *hdr);
  const u32 stored = (u32)host[CH_STORED];
  if (stored) memcpy(recs, host.data() + SIM_CENSUS_WORDS, (size_t)stored * sizeof *recs);
  *n = stored;
  return SIM_OK;
}

}  // extern "C"
