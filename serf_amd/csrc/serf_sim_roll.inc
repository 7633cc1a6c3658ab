// serf_sim_roll.inc — part of the translation unit serf_sim.hip (included from there, after the census; not a header of its own).
// Observer roll (include/serf_sim_roll.h): four kernels behind a sampled tick's last launch, the host's bookkeeping, the entry points.
//
// Per sampled tick:
//   census_count_kernel, census_fold_kernel   (serf_sim_census.inc, as they are) into scratch of the roll's own: per allocated slot the
//                        subject's record — of it the roll reads ltmax, incmax, "any observer knows it" and the subject's own liveness
//   roll_count_kernel    the transposed sweep: an observer per lane, a workgroup per BLOCK nodes, no pass loop (the grid grows with the
//                        handle: 65 536 workgroups at the 16 Mi nodes a handle can have).  The slots 0 .. bound - 1 (the host's high-water
//                        mark) go by in chunks of ROLL_CHUNK: the workgroup asks subject_of on the device which of a chunk hold a subject —
//                        slots are handed out and given back while sim_step(h, n) runs ahead — compacts those into LDS next to their
//                        reference records (the same list in every lane), and then every lane loads ITS entry of each listed slot: one
//                        16-byte head load per (slot, lane), 1 KiB per wave and instruction, in batches of ROLL_BATCH independent loads.
//                        The tail plane is never touched, a free slot's plane — which may have no memory — never read.  Whether the
//                        observer runs is a bit of upmap.  The six counts and lag stay in the lane's registers: an observer's record
//                        needs no cross-lane step.  Behind the sweep the header's sums, maxima and bins go through LDS into the
//                        workgroup's column of a partial matrix — integers throughout, no atomics on global memory, nothing to zero —
//                        and the workgroup lists its own top_k candidates (rank_candidates, serf_sim_observe.inc) by key = score << 32 |
//                        (0xFFFFFFFF - id): keys are unique.  A candidate carries its key and all eight words of the record.
//                        sim_roll_now may ask for every node's record: then the lane stores its 64 bytes as well; a sampled roll
//                        writes no per-node array
//   roll_fold_kernel     one workgroup: folds the partial rows into the header, counts the subjects, merges the workgroups' candidate
//                        lists (rank_merge) and writes the listed records, zeroing what stays unused
// Their order is the stream's.  The host knows every sampled tick in advance: it passes the sample's place to the launches and reads nothing back.
// A handle without a started roll never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_roll.h"

static_assert(sizeof(sim_roll_node) == 64 && sizeof(sim_roll_header) == 256 && SIM_ROLL_NODE_WORDS == 8u && SIM_ROLL_HEADER_WORDS == 32u,
              "layout of include/serf_sim_roll.h");
static_assert(SIM_ROLL_TOP_MAX <= BLOCK, "a workgroup has top_k candidates at most among its BLOCK observers");

#define ROLL_CHUNK 256u  // slots a workgroup looks at per pass over subject_of: a lane each
#define ROLL_BATCH 8u    // independent head loads in flight a lane (8 x 4 registers, as in census_count_kernel)
static_assert(ROLL_CHUNK == BLOCK && ROLL_CHUNK % ROLL_BATCH == 0u, "a lane stages one slot of a chunk");
// words of a node's record and of the header (include/serf_sim_roll.h)
enum { RW_ID = 0, RW_STALE = 1, RW_UNKNOWN = 2, RW_FF = 3, RW_SUSP = 4, RW_SA = 5, RW_LAG = 6, RW_BEHIND = 7 };
enum { RH_TICK = 0, RH_UP = 1, RH_SUBJECTS = 2, RH_LISTED = 3, RH_CURRENT = 4, RH_STALE_SUM = 5, RH_STALE_MAX = 6, RH_UNKNOWN_SUM = 7,
       RH_FF_OBS = 8, RH_FF_SUM = 9, RH_SUSP_OBS = 10, RH_SUSP_SUM = 11, RH_SA_OBS = 12, RH_SA_SUM = 13, RH_LAG_SUM = 14, RH_LAG_MAX = 15,
       RH_BIN = 16 };
__host__ __device__ static inline u32 roll_op(u32 w) { return (w == RH_STALE_MAX || w == RH_LAG_MAX) ? FOLD_MAX : FOLD_SUM; }
// words 0, 2 and 3 are the fold kernel's own; every other word has a row of partial results
__host__ __device__ static inline bool roll_has_row(u32 w) { return w == RH_UP || w >= RH_CURRENT; }

struct RollDevP {
  const uint4* view;      // Dev::view: the head planes, [A][Nl]
  const u32* subject_of;  // Dev::subject_of
  const u32* upmap;       // Dev::upmap
  const u64* rec;         // [bound][SIM_CENSUS_WORDS]: census_fold_kernel's record of every allocated slot
  u64* part;              // [SIM_ROLL_HEADER_WORDS][G]: every workgroup of the count kernel writes its column
  u64* ckey;              // [G][top_k]: a workgroup's candidates, descending; key 0 ends a list that is shorter
  u64* crec;              // [G][top_k][SIM_ROLL_NODE_WORDS]: their records
  u64* nodes;             // null, or [N][SIM_ROLL_NODE_WORDS]: every node's record (sim_roll_now)
  u64* out;               // the sample: a header, then top_k records
  u32 N, Nl;
  u32 G;                  // workgroups of the count kernel: ceil(Nl / BLOCK)
  u32 bound;              // slots 0 .. bound - 1 are looked at (the host's high-water mark; which of them are allocated the device decides)
  u32 top_k, rank_by;
  u32 now;                // sim_tick after the sampled tick
};

__device__ static inline u64 roll_score(const u64 w[SIM_ROLL_NODE_WORDS], u32 rank_by) {
  return rank_by == SIM_ROLL_BY_STALE ? w[RW_STALE] : rank_by == SIM_ROLL_BY_ACCUSED ? w[RW_FF] + w[RW_SUSP] : w[RW_SA];
}
__global__ __launch_bounds__(BLOCK) void roll_count_kernel(RollDevP p) {
  __shared__ u32 s_slot[ROLL_CHUNK];   // the chunk's allocated slots, ascending
  __shared__ u64 s_ltmax[ROLL_CHUNK];  // their references
  __shared__ u32 s_incmax[ROLL_CHUNK];
  __shared__ u32 s_flags[ROLL_CHUNK];  // bit 0: some observer knows the subject; bit 1: the subject's own process runs
  __shared__ u32 s_wcnt[BLOCK / 64];
  __shared__ unsigned long long acc[SIM_ROLL_HEADER_WORDS];
  __shared__ u64 red[2][BLOCK / 64];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;  // the observer
  const bool in = i < p.Nl && i < p.N;
  const bool up = in && ((p.upmap[i >> 5] >> (i & 31u)) & 1u);
  const u32 li = min(i, p.Nl - 1u);  // (lanes beyond the last node: its entry once more, not counted — the batch's loads stay unconditional)
  if (threadIdx.x < SIM_ROLL_HEADER_WORDS) acc[threadIdx.x] = 0;
  u32 unknown = 0, behind = 0, ff = 0, susp = 0, sa = 0;
  u64 lag = 0;
#pragma unroll 1
  for (u32 a0 = 0; a0 < p.bound; a0 += ROLL_CHUNK) {  // (whole workgroups stay together: the barriers below)
    const u32 a = a0 + threadIdx.x;
    const bool alloc = a < p.bound && p.subject_of[a] != NOSLOT;
    const u64 bal = __ballot(alloc);
    __syncthreads();  // (the lists of the chunk before have been read)
    if (!lane) s_wcnt[wave] = (u32)__popcll(bal);
    __syncthreads();
    u32 off = 0, cnt = 0;
#pragma unroll
    for (u32 q = 0; q < BLOCK / 64; ++q) { off += q < wave ? s_wcnt[q] : 0u; cnt += s_wcnt[q]; }
    if (alloc) {
      const u32 r = off + (u32)__popcll(bal & ((1ull << lane) - 1ull));
      const u64* src = p.rec + (size_t)a * SIM_CENSUS_WORDS;
      const bool anyknown = (src[CW_SWIM] | src[CW_SWIM + 1] | src[CW_SWIM + 2] | src[CW_SWIM + 3]) != 0;  // (the swim bins: the known observers)
      s_slot[r] = a;
      s_ltmax[r] = src[CW_LTMAX];
      s_incmax[r] = (u32)src[CW_INCMAX];
      s_flags[r] = (anyknown ? 1u : 0u) | ((src[CW_UP] & 1u) ? 2u : 0u);
    }
    __syncthreads();
#pragma unroll 1
    for (u32 k0 = 0; k0 < cnt; k0 += ROLL_BATCH) {  // (cnt is the same in every lane)
      uint4 e[ROLL_BATCH];
#pragma unroll
      for (u32 j = 0; j < ROLL_BATCH; ++j) {
        const u32 k = min(k0 + j, cnt - 1u);  // (beyond the list's end: its last slot once more, not counted)
        e[j] = ld4(&p.view[(size_t)s_slot[k] * p.Nl + li]);
      }
#pragma unroll
      for (u32 j = 0; j < ROLL_BATCH; ++j) {
        const u32 k = min(k0 + j, cnt - 1u);
        const bool counted = k0 + j < cnt;
        const u64 ltmax = s_ltmax[k];
        const u32 incmax = s_incmax[k], fl = s_flags[k];
        const u32 bits = e[j].w;
        const bool known = counted && (bits & SIM_VB_KNOWN);
        const bool run = fl & 2u;
        const u32 st = SIM_VB_STATUS(bits), sw = SIM_VB_SWIM(bits);
        const u64 lt = (u64)e[j].x | ((u64)e[j].y << 32);
        unknown += (counted && !(bits & SIM_VB_KNOWN) && (fl & 1u)) ? 1u : 0u;
        behind += (known && (lt < ltmax || e[j].z < incmax)) ? 1u : 0u;
        ff += (known && run && st == SIM_STATUS_FAILED) ? 1u : 0u;
        susp += (known && run && (sw == SIM_SWIM_SUSPECT || sw == SIM_SWIM_DEAD)) ? 1u : 0u;
        sa += (known && !run && st == SIM_STATUS_ALIVE) ? 1u : 0u;
        lag += known ? ltmax - lt : 0ull;
      }
    }
  }
  // the observer's record (a node that does not run observes nothing)
  u64 w[SIM_ROLL_NODE_WORDS];
  w[RW_ID] = (u64)i | ((u64)(up ? 1u : 0u) << 32);
  w[RW_STALE] = up ? (u64)unknown + behind : 0ull;
  w[RW_UNKNOWN] = up ? unknown : 0u;
  w[RW_FF] = up ? ff : 0u;
  w[RW_SUSP] = up ? susp : 0u;
  w[RW_SA] = up ? sa : 0u;
  w[RW_LAG] = up ? lag : 0ull;
  w[RW_BEHIND] = up ? behind : 0u;
  if (p.nodes && in) {
    u64* dst = p.nodes + (size_t)i * SIM_ROLL_NODE_WORDS;
#pragma unroll
    for (u32 k = 0; k < SIM_ROLL_NODE_WORDS; ++k) dst[k] = w[k];
  }
  // the header's words: the wave's share into LDS, the workgroup's column of the partial matrix
  __syncthreads();  // (acc is zero; with bound == 0 no barrier stood behind that)
  {
    const u64 stale = w[RW_STALE];
    const u64 sums[10] = {up ? 1ull : 0ull, (up && !stale) ? 1ull : 0ull, stale, w[RW_UNKNOWN], w[RW_FF] ? 1ull : 0ull, w[RW_FF],
                          w[RW_SUSP] ? 1ull : 0ull, w[RW_SUSP], w[RW_SA] ? 1ull : 0ull, w[RW_SA]};
    const u32 word[10] = {RH_UP, RH_CURRENT, RH_STALE_SUM, RH_UNKNOWN_SUM, RH_FF_OBS, RH_FF_SUM, RH_SUSP_OBS, RH_SUSP_SUM, RH_SA_OBS, RH_SA_SUM};
#pragma unroll
    for (u32 k = 0; k < 10; ++k) {
      const u64 t = wave_sum(sums[k]);
      if (!lane && t) atomicAdd(&acc[word[k]], (unsigned long long)t);  // (LDS)
    }
    const u64 lsum = wave_sum(w[RW_LAG]), lmax = wave_max(w[RW_LAG]), smax = wave_max(stale);
    if (!lane) {
      if (lsum) atomicAdd(&acc[RH_LAG_SUM], (unsigned long long)lsum);
      atomicMax(&acc[RH_LAG_MAX], (unsigned long long)lmax);
      atomicMax(&acc[RH_STALE_MAX], (unsigned long long)smax);
    }
    // bin 0: stale == 0; otherwise 1 + floor(log2(stale)), 15 at most
    const u32 bin = stale ? min(1u + (31u - (u32)__clz((u32)stale)), 15u) : 0u;
#pragma unroll
    for (u32 b = 0; b < 16; ++b) {
      const u64 m = __ballot(up && bin == b);
      if (!lane && m) atomicAdd(&acc[RH_BIN + b], (unsigned long long)__popcll(m));
    }
  }
  __syncthreads();
  if (threadIdx.x < SIM_ROLL_HEADER_WORDS && roll_has_row(threadIdx.x)) p.part[(size_t)threadIdx.x * p.G + blockIdx.x] = acc[threadIdx.x];
  // the workgroup's candidates
  const u64 score = roll_score(w, p.rank_by);  // (0 for a node that does not run: never listed)
  const u64 key = score ? (score << 32) | (u64)(0xFFFFFFFFu - i) : 0ull;
  rank_candidates<SIM_ROLL_NODE_WORDS>(key, w, p.ckey, p.crec, p.top_k, red);
}

// one workgroup: the header out of the partial rows, the listed records out of the workgroups' candidates
__global__ __launch_bounds__(BLOCK) void roll_fold_kernel(RollDevP p) {
  __shared__ unsigned long long hdr[SIM_ROLL_HEADER_WORDS];
  __shared__ u64 red[2][BLOCK / 64];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < SIM_ROLL_HEADER_WORDS) hdr[threadIdx.x] = 0;
  __syncthreads();
  for (u32 w = wave; w < SIM_ROLL_HEADER_WORDS; w += BLOCK / 64) {  // a wave per word
    if (!roll_has_row(w)) continue;
    const u64 v = fold_row(p.part + (size_t)w * p.G, p.G, roll_op(w));
    if (!lane) hdr[w] = v;
  }
  {  // the subjects: bound words of subject_of
    u32 c = 0;
    for (u32 a = threadIdx.x; a < p.bound; a += BLOCK) c += p.subject_of[a] != NOSLOT ? 1u : 0u;
    c = (u32)wave_sum(c);
    if (!lane && c) atomicAdd(&hdr[RH_SUBJECTS], (unsigned long long)c);  // (LDS)
  }
  const u32 r = rank_merge<SIM_ROLL_NODE_WORDS>(p.ckey, p.crec, p.G, p.top_k, p.out + SIM_ROLL_HEADER_WORDS, red, FillZero());
  if (threadIdx.x == 0) {
    hdr[RH_TICK] = p.now;
    hdr[RH_LISTED] = (u64)r | ((u64)p.rank_by << 32);
  }
  __syncthreads();
  if (threadIdx.x < SIM_ROLL_HEADER_WORDS) p.out[threadIdx.x] = hdr[threadIdx.x];
}

// ---- host ----
// what the kernels need besides the sample's place, for every slot the handle can ever hand out and a given top_k
struct RollScratch {
  DevScratch<u64> d_cpart, d_crec;  // the census kernels' scratch (census_scratch)
  DevScratch<u64> d_part;           // [SIM_ROLL_HEADER_WORDS][G]
  DevScratch<u64> d_ckey, d_crec2;  // [G][top_k], [G][top_k][SIM_ROLL_NODE_WORDS]
};
static inline u32 roll_groups(const sim_handle* h) { return (h->d.Nl + BLOCK - 1u) / BLOCK; }
static inline size_t roll_stride(u32 top_k) { return SIM_ROLL_HEADER_WORDS + (size_t)top_k * SIM_ROLL_NODE_WORDS; }  // words of a sample
static inline bool roll_args_ok(u32 top_k, u32 rank_by) { return top_k >= 1u && top_k <= SIM_ROLL_TOP_MAX && rank_by <= SIM_ROLL_BY_MISSED; }

static int roll_scratch(const sim_handle* h, RollScratch& s, u32 top_k) {
  const size_t G = roll_groups(h);
  if (int rc = census_scratch(h, s.d_cpart, s.d_crec)) return rc;
  if (int rc = s.d_part.alloc(G * SIM_ROLL_HEADER_WORDS)) return rc;
  if (int rc = s.d_ckey.alloc(G * top_k)) return rc;
  return s.d_crec2.alloc(G * top_k * SIM_ROLL_NODE_WORDS);
}
// one roll of the state the stream will be in when it gets here, into out[roll_stride(top_k)]; nodes: null, or [N] records
static int roll_launch(sim_handle* h, const RollScratch& s, u64* out, u64* nodes, u32 top_k, u32 rank_by) {
  const CenDevP c = census_records(h, s.d_cpart.get(), s.d_crec.get(), nullptr, 0);
  RollDevP p;
  p.view = c.view; p.subject_of = c.subject_of; p.upmap = c.upmap;
  p.rec = c.rec; p.part = s.d_part.get(); p.ckey = s.d_ckey.get(); p.crec = s.d_crec2.get();
  p.nodes = nodes; p.out = out;
  p.N = c.N; p.Nl = c.Nl;
  p.G = roll_groups(h);
  p.bound = c.bound;
  p.top_k = top_k; p.rank_by = rank_by;
  p.now = c.now;
  roll_count_kernel<<<p.G, BLOCK, 0, h->stream>>>(p);
  roll_fold_kernel<<<1, BLOCK, 0, h->stream>>>(p);
  HCHECK(hipGetLastError());
  return SIM_OK;
}
struct RollState : Observer {  // samples of SIM_ROLL_HEADER_WORDS + top_k * SIM_ROLL_NODE_WORDS words
  RollScratch scr;
  u32 top_k = 0, rank_by = 0;
  int sample(sim_handle* h, u64* out) override { return roll_launch(h, scr, out, nullptr, top_k, rank_by); }
};

extern "C" {

uint32_t sim_roll_version(void) { return SIM_ROLL_VERSION; }

int sim_roll_start(sim_handle* h, uint32_t first_tick, uint32_t period, uint32_t capacity, uint32_t top_k, uint32_t rank_by) {
  RollState* s = new RollState();
  s->top_k = top_k;
  s->rank_by = rank_by;
  return observer_start(h, OB_ROLL, s, SIM_ROLL_MAX_SAMPLES, first_tick, period, capacity, roll_stride(top_k),
                        [&] { return roll_args_ok(top_k, rank_by) ? SIM_OK : SIM_EINVAL; }, [&] { return roll_scratch(h, s->scr, top_k); });
}

int sim_roll_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_ROLL, taken, dropped); }

int sim_roll_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_ROLL, first, n, out, cap_words, n_out);
}

int sim_roll_stop(sim_handle* h) { return observer_stop(h, OB_ROLL); }

int sim_roll_now(sim_handle* h, uint32_t top_k, uint32_t rank_by, sim_roll_header* hdr, sim_roll_node* top, sim_roll_node* nodes) {
  if (int rc = observer_usable(h)) return rc;
  if (!hdr || !top || !roll_args_ok(top_k, rank_by)) return SIM_EINVAL;
  // scratch of its own: a running roll's candidate arrays are sized for ITS top_k, and its samples still enqueued use them
  RollScratch own;
  DevScratch<u64> d_nodes;
  std::vector<u64> host(roll_stride(top_k));
  int rc = roll_scratch(h, own, top_k);
  if (rc == SIM_OK && nodes) rc = d_nodes.alloc((size_t)h->d.N * SIM_ROLL_NODE_WORDS);
  if (rc != SIM_OK) return rc;
  rc = observer_now(h, host.size(), host.data(), [&](u64* out) { return roll_launch(h, own, out, nodes ? d_nodes.get() : nullptr, top_k, rank_by); });
  if (rc != SIM_OK) return rc;
  if (nodes) HCHECK(hipMemcpy(nodes, d_nodes.get(), (size_t)h->d.N * sizeof *nodes, hipMemcpyDeviceToHost));
  memcpy(hdr, host.data(), sizeof *hdr);
  memcpy(top, host.data() + SIM_ROLL_HEADER_WORDS, (size_t)top_k * sizeof *top);
  return SIM_OK;
}

}  // extern "C"
