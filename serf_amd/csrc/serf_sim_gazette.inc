// serf_sim_gazette.inc — part of the translation unit serf_sim.hip (included from there, behind the catalogue; not a header of its own).
// Member gazette (include/serf_sim_gazette.h): the kernels behind a sampled tick's last launch, the host's bookkeeping, the entry points.
//
// Per sampled tick:
//   gazette_scan_kernel  the roll's layout (roll_count_kernel): a node per lane, a workgroup per BLOCK nodes, GAZETTE_GRID workgroups at
//                        most and a pass loop over the blocks of nodes beyond, whole workgroups kept together.  The slots 0 .. bound - 1
//                        (the host's high-water mark) go by in chunks of GZ_CHUNK: the workgroup asks subject_of on the device which of
//                        a chunk hold a subject, compacts those into LDS next to "is the slot fresh", the baseline's bits of a fresh one
//                        and where its shadow row lies, and then every lane loads, per listed slot, the `bits` word of ITS head entry
//                        and ITS shadow word: two coalesced 4-byte loads, GZ_BATCH slots in flight.  "No lane of the wave differs from
//                        its shadow" costs those two loads, the reads of the slot's list entry from LDS, one compare and one ballot.  A wave with a lane that differs stores the
//                        shadow where it differs, classifies the transition, keeps the node's seven counts in registers, adds the
//                        popcounts of seven ballots to the chunk's table in LDS (GZ_CHUNK x 8 words, 4 KiB) and the matrices' cells to
//                        the workgroup's accumulators in LDS.  Behind a chunk the table goes to the workgroup's column of the partial
//                        counts part[slot][column][workgroup] — written in the first pass, added to by the SAME workgroup in later ones:
//                        no atomics on global memory, nothing to zero.  Behind a pass a node that saw anything adds its counts to its
//                        row of the node map (its own row: nobody else writes it).  The tail plane is never touched, a free slot's
//                        plane — which may have no memory — never read.
//   gazette_fold_kernel  a wave per slot below the highest bound the gazette has seen: adds the workgroups' partial counts up, adds them
//                        to the subject's row of the subject map (a subject owns one slot: nobody else writes the row), moves its peak,
//                        leaves the slot's record (seven sums, allocated / fresh) for the pack kernel and sets shadow_subject — also
//                        for a slot that is free now, whose entry is cleared
//   gazette_pack_kernel  one workgroup: the matrices, the histogram and the nodes' extremes out of the workgroups' rows, the sums and the
//                        subjects' extremes out of the slots' records, the running nodes out of upmap; writes the sample
//   gazette_shadow_kernel  sim_gazette_start, and the first sample behind a restore: the whole shadow := the heads' bits; the fold kernel
//                        then marks every allocated slot fresh and counts nothing
// Their order is the stream's.  The host knows every sampled tick in advance: it passes the sample's place to the launches and reads nothing back.
// A handle without a started gazette never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_gazette.h"

static_assert(sizeof(sim_gazette_sample) == 512 && sizeof(sim_gazette_row) == 32 && sizeof(sim_gazette_rank) == 40 && SIM_GAZETTE_COLS == 8u,
              "layout of include/serf_sim_gazette.h");
static_assert(SIM_GAZETTE_TOP_MAX <= BLOCK, "a workgroup has top_k candidates at most among its BLOCK rows");
static_assert(SIM_STATUS_FAILED == 4 && SIM_SWIM_LEFT == 3, "a 5 x 5 and a 4 x 4 matrix");

#define GAZETTE_GRID 1024u  // workgroups of the scan kernel at most
#define GZ_CHUNK 128u       // slots a workgroup looks at per pass over subject_of: 4 KiB of counts in LDS
#define GZ_BATCH 8u         // slots whose two loads are in flight a lane (16 registers)
#define GZ_GROUPS 64u       // the shadow is allocated in at most so many groups of slots
#define GZ_RANK_WORDS 5u    // sim_gazette_rank
static_assert(GZ_CHUNK <= BLOCK && GZ_CHUNK % GZ_BATCH == 0u, "a lane stages one slot of a chunk");
// rows of the scan kernel's partial results [GZ_ROWS][G]; a sample's words 4 .. 44 are rows 0 .. 40
enum { GZ_MAT = 0, GZ_SWIM = 25, GZ_HIST = 41, GZ_NODES = 46, GZ_MAXKEY = 47, GZ_ROWS = 48 };
// words of a sample
enum { GW_TICK = 0, GW_UP = 1, GW_SLOTS = 2, GW_FRESH = 3, GW_MAT = 4, GW_SWIM = 29, GW_SUMS = 45, GW_NODES = 52, GW_NODE_MAX = 53,
       GW_NODE_ID = 54, GW_SUBJECTS = 55, GW_SUBJ_ID = 56, GW_SUBJ_MAX = 57, GW_HIST = 58 };
static_assert(GW_MAT + GZ_SWIM == GW_SWIM && GZ_ROWS <= BLOCK, "the matrices' rows are the sample's words, four on");

struct GazDevP {
  const uint4* view;      // Dev::view: the head planes, [A][Nl]
  const u32* subject_of;  // Dev::subject_of
  const u32* upmap;       // Dev::upmap
  const uint4* base;      // [N][2]: the subjects' baseline entries
  u32* const* grp;        // [GZ_GROUPS]: the shadow's groups, [gslots][Nl] each; slot a is row a % gslots of group a / gslots
  u32* shsub;             // [A]: shadow_subject
  u32* nodes;             // [N][8]: the node map
  u32* subj;              // [N][8]: the subject map
  u32* part;              // [cap][8][G]: the scan kernel's counts of every (slot, column, workgroup)
  u64* hpart;             // [GZ_ROWS][G]: its other results, a column a workgroup
  u32* srec;              // [cap][8]: the fold kernel's record of a slot: seven sums, then bit 0 allocated, bit 1 fresh
  u64* out;               // the sample
  u32 N, Nl;
  u32 G;                  // workgroups of the scan kernel
  u32 bound;              // slots 0 .. bound - 1 are looked at (the host's high-water mark; which of them are allocated the device decides)
  u32 range;              // the highest bound any sample has seen (>= bound): the fold's range, so that a slot freed above the bound is cleared
  u32 gslots;             // slots a group holds
  u32 t, now;             // the sampled tick, sim_tick after it
  u32 window;             // flap_window
  u32 rebase;             // the shadow was re-taken: every allocated slot is fresh, nothing is counted
};

__device__ static inline u32 gz_state(u32 bits) { return (bits & SIM_VB_KNOWN) ? min(SIM_VB_STATUS(bits), (u32)SIM_STATUS_FAILED) : 0u; }

__global__ __launch_bounds__(BLOCK) void gazette_scan_kernel(GazDevP p) {
  __shared__ u32 s_slot[GZ_CHUNK];     // the chunk's allocated slots, ascending
  __shared__ u32 s_fresh[GZ_CHUNK];    // shadow_subject is not the slot's subject
  __shared__ u32 s_base[GZ_CHUNK];     // ... then the bits of the subject's baseline
  __shared__ u32* s_row[GZ_CHUNK];     // the slots' shadow rows
  __shared__ u32 s_cnt[GZ_CHUNK][SIM_GAZETTE_COLS];
  __shared__ u32 s_wcnt[BLOCK / 64];
  __shared__ unsigned long long acc[GZ_ROWS];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < GZ_ROWS) acc[threadIdx.x] = 0;
  __syncthreads();
  u32 pass = 0;
#pragma unroll 1
  for (u32 nb = blockIdx.x; (size_t)nb * BLOCK < p.Nl; nb += gridDim.x, ++pass) {  // (whole workgroups stay together: the barriers below)
    const u32 i = nb * BLOCK + threadIdx.x;  // the observer
    const bool in = i < p.Nl && i < p.N;
    const bool up = in && ((p.upmap[i >> 5] >> (i & 31u)) & 1u);
    const u32 li = min(i, p.Nl - 1u);  // (lanes beyond the last node: its entry once more, neither counted nor stored)
    u32 c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0;
#pragma unroll 1
    for (u32 a0 = 0; a0 < p.bound; a0 += GZ_CHUNK) {
      const u32 a = a0 + threadIdx.x;
      const u32 x = (threadIdx.x < GZ_CHUNK && a < p.bound) ? p.subject_of[a] : NOSLOT;
      const bool alloc = x != NOSLOT;
      const u64 bal = __ballot(alloc);
      __syncthreads();  // (the lists and the table of the chunk before have been read)
      if (!lane) s_wcnt[wave] = (u32)__popcll(bal);
      for (u32 k = threadIdx.x; k < GZ_CHUNK * SIM_GAZETTE_COLS; k += BLOCK) (&s_cnt[0][0])[k] = 0;
      __syncthreads();
      u32 off = 0, cnt = 0;
#pragma unroll
      for (u32 q = 0; q < BLOCK / 64; ++q) { off += q < wave ? s_wcnt[q] : 0u; cnt += s_wcnt[q]; }
      if (alloc) {
        const u32 r = off + (u32)__popcll(bal & ((1ull << lane) - 1ull));
        const bool fresh = p.shsub[a] != x;
        const u32 g = a / p.gslots;
        s_slot[r] = a;
        s_fresh[r] = fresh ? 1u : 0u;
        s_base[r] = fresh ? p.base[(size_t)x * 2].w : 0u;
        s_row[r] = p.grp[g] + (size_t)(a - g * p.gslots) * p.Nl;
      }
      __syncthreads();
#pragma unroll 1
      for (u32 k0 = 0; k0 < cnt; k0 += GZ_BATCH) {  // (cnt is the same in every lane)
        u32 cur[GZ_BATCH], sh[GZ_BATCH];
#pragma unroll
        for (u32 j = 0; j < GZ_BATCH; ++j) {
          const u32 k = min(k0 + j, cnt - 1u);  // (beyond the list's end: its last slot once more, not counted)
          cur[j] = p.view[(size_t)s_slot[k] * p.Nl + li].w;
          sh[j] = s_row[k][li];
        }
#pragma unroll
        for (u32 j = 0; j < GZ_BATCH; ++j) {
          const u32 k = min(k0 + j, cnt - 1u);
          const bool fresh = s_fresh[k];
          const bool diff = in && k0 + j < cnt && (fresh || cur[j] != sh[j]);
          if (!__ballot(diff)) continue;  // nobody in the wave has news of this subject
          const u32 prev = fresh ? s_base[k] : sh[j];
          if (diff) s_row[k][i] = cur[j];  // (in: i < Nl)
          const bool ch = up && diff && cur[j] != prev;
          const u32 sp = gz_state(prev), sc = gz_state(cur[j]);
          const bool gone = sp == SIM_STATUS_LEFT || sp == SIM_STATUS_FAILED;
          const bool join = ch && ((sp == 0u && sc != 0u) || (gone && sc == SIM_STATUS_ALIVE));
          const bool leave = ch && sc == SIM_STATUS_LEFT && sp != 0u && sp != SIM_STATUS_LEFT;
          const bool failed = ch && sc == SIM_STATUS_FAILED && sp != 0u && sp != SIM_STATUS_FAILED;
          const bool reap = ch && sp != 0u && sc == 0u;
          const bool back = ch && sp == SIM_STATUS_FAILED && sc == SIM_STATUS_ALIVE;  // a join out of Failed
          const u32 age = (p.t - SIM_VB_STAMP(prev)) & STAMP_MASK;
          const bool flap = back && age < p.window;
          const bool both = ch && (prev & cur[j] & SIM_VB_KNOWN);
          const u32 wp = SIM_VB_SWIM(prev), wc = SIM_VB_SWIM(cur[j]);
          const bool susp = both && wp == SIM_SWIM_ALIVE && wc == SIM_SWIM_SUSPECT;
          const bool clr = both && wp == SIM_SWIM_SUSPECT && wc == SIM_SWIM_ALIVE;
          c0 += join ? 1u : 0u; c1 += leave ? 1u : 0u; c2 += failed ? 1u : 0u; c3 += reap ? 1u : 0u;
          c4 += flap ? 1u : 0u; c5 += susp ? 1u : 0u; c6 += clr ? 1u : 0u;
          {  // the subject's counts: seven ballots, lane q adds the popcount of column q (LDS)
            const u64 b0 = __ballot(join), b1 = __ballot(leave), b2 = __ballot(failed), b3 = __ballot(reap), b4 = __ballot(flap),
                      b5 = __ballot(susp), b6 = __ballot(clr);
            const u64 mine = lane == 0 ? b0 : lane == 1 ? b1 : lane == 2 ? b2 : lane == 3 ? b3 : lane == 4 ? b4 : lane == 5 ? b5 : b6;
            if (lane < 7u && mine) atomicAdd(&s_cnt[k][lane], (u32)__popcll(mine));
          }
          if (ch && sp != sc) atomicAdd(&acc[GZ_MAT + sp * 5u + sc], 1ull);  // (LDS; sp, sc <= 4)
          if (both && wp != wc) atomicAdd(&acc[GZ_SWIM + wp * 4u + wc], 1ull);
          if (back) atomicAdd(&acc[GZ_HIST + (age < 2u ? 0u : age < 8u ? 1u : age < 32u ? 2u : age < 128u ? 3u : 4u)], 1ull);
        }
      }
      __syncthreads();  // (the chunk's table is complete)
      for (u32 k = threadIdx.x; k < cnt * SIM_GAZETTE_COLS; k += BLOCK) {
        u32* dst = p.part + ((size_t)s_slot[k >> 3] * SIM_GAZETTE_COLS + (k & 7u)) * p.G + blockIdx.x;
        const u32 v = s_cnt[k >> 3][k & 7u];
        *dst = pass ? *dst + v : v;  // (this workgroup's own column: the first pass writes it, the later ones add)
      }
    }
    // the node's row of the node map, when it saw anything
    const u32 ev = c0 + c1 + c2 + c3;
    if (in && (ev | c4 | c5 | c6)) {
      uint4* row = reinterpret_cast<uint4*>(p.nodes + (size_t)i * SIM_GAZETTE_COLS);
      uint4 lo = row[0], hi = row[1];
      lo.x += c0; lo.y += c1; lo.z += c2; lo.w += c3;
      hi.x += c4; hi.y += c5; hi.z += c6; hi.w = max(hi.w, ev);
      row[0] = lo; row[1] = hi;
    }
    lds_sum(&acc[GZ_NODES], ev ? 1ull : 0ull);
    lds_max(&acc[GZ_MAXKEY], ev ? ((u64)ev << 32) | (u64)(0xFFFFFFFFu - i) : 0ull);  // (the lowest id of the largest count)
  }
  __syncthreads();
  if (threadIdx.x < GZ_ROWS) p.hpart[(size_t)threadIdx.x * p.G + blockIdx.x] = acc[threadIdx.x];
}

// the whole shadow := the heads' bits of every allocated slot below the bound
__global__ __launch_bounds__(BLOCK) void gazette_shadow_kernel(GazDevP p) {
#pragma unroll 1
  for (u32 nb = blockIdx.x; (size_t)nb * BLOCK < p.Nl; nb += gridDim.x) {
    const u32 i = nb * BLOCK + threadIdx.x;
    if (i >= p.Nl) continue;
    for (u32 a = 0; a < p.bound; ++a) {
      if (p.subject_of[a] == NOSLOT) continue;  // (the same in every lane; a free slot's plane is not read)
      const u32 g = a / p.gslots;
      (p.grp[g] + (size_t)(a - g * p.gslots) * p.Nl)[i] = p.view[(size_t)a * p.Nl + i].w;
    }
  }
}

// a wave per slot: the workgroups' counts added up, the subject's row of the subject map, the slot's record, shadow_subject
__global__ __launch_bounds__(BLOCK) void gazette_fold_kernel(GazDevP p) {
  const u32 a = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (a >= p.range) return;  // (whole waves)
  u32* rec = p.srec + (size_t)a * SIM_GAZETTE_COLS;
  const u32 x = p.subject_of[a];
  const u32 was = p.shsub[a];
  if (x == NOSLOT || a >= p.bound) {  // free: only its shadow_subject is cleared
    if (lane < SIM_GAZETTE_COLS) rec[lane] = 0;
    if (!lane && was != NOSLOT) p.shsub[a] = NOSLOT;
    return;
  }
  const bool fresh = p.rebase || was != x;
  u32 s[7] = {0, 0, 0, 0, 0, 0, 0};
  if (!p.rebase) {
#pragma unroll
    for (u32 k = 0; k < 7; ++k) s[k] = (u32)fold_row(p.part + ((size_t)a * SIM_GAZETTE_COLS + k) * p.G, p.G, FOLD_SUM);
  }
  if (lane) return;
  if (was != x) p.shsub[a] = x;
#pragma unroll
  for (u32 k = 0; k < 7; ++k) rec[k] = s[k];
  rec[7] = 1u | (fresh ? 2u : 0u);
  if (s[0] | s[1] | s[2] | s[3] | s[4] | s[5] | s[6]) {
    u32* m = p.subj + (size_t)x * SIM_GAZETTE_COLS;
#pragma unroll
    for (u32 k = 0; k < 7; ++k) m[k] += s[k];
    m[7] = max(m[7], s[2]);
  }
}

// one workgroup: the sample
__global__ __launch_bounds__(BLOCK) void gazette_pack_kernel(GazDevP p) {
  __shared__ unsigned long long hdr[SIM_GAZETTE_WORDS];
  __shared__ unsigned long long kmax[2];  // the nodes' and the subjects' largest key
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < SIM_GAZETTE_WORDS) hdr[threadIdx.x] = 0;
  if (threadIdx.x < 2) kmax[threadIdx.x] = 0;
  __syncthreads();
  if (!p.rebase) {
    for (u32 r = wave; r < GZ_ROWS; r += BLOCK / 64) {  // a wave per row
      const u64 v = fold_row(p.hpart + (size_t)r * p.G, p.G, r == GZ_MAXKEY ? FOLD_MAX : FOLD_SUM);
      if (lane) continue;
      if (r < GZ_HIST) hdr[GW_MAT + r] = v;
      else if (r < GZ_NODES) hdr[GW_HIST + (r - GZ_HIST)] = v;
      else if (r == GZ_NODES) hdr[GW_NODES] = v;
      else kmax[0] = v;
    }
  }
  {  // the slots' records
    u64 looked = 0, fresh = 0, subjects = 0, key = 0, sum[7] = {0, 0, 0, 0, 0, 0, 0};
    for (u32 a = threadIdx.x; a < p.bound; a += BLOCK) {
      const u32* rec = p.srec + (size_t)a * SIM_GAZETTE_COLS;
      const u32 fl = rec[7];
      if (!(fl & 1u)) continue;
      looked++;
      fresh += (fl >> 1) & 1u;
#pragma unroll
      for (u32 k = 0; k < 7; ++k) sum[k] += rec[k];
      subjects += (rec[0] | rec[1] | rec[2] | rec[3]) ? 1u : 0u;
      const u64 kk = rec[2] ? ((u64)rec[2] << 32) | (u64)(0xFFFFFFFFu - p.subject_of[a]) : 0ull;
      key = kk > key ? kk : key;
    }
    lds_sum(&hdr[GW_SLOTS], looked);
    lds_sum(&hdr[GW_FRESH], fresh);
    lds_sum(&hdr[GW_SUBJECTS], subjects);
#pragma unroll
    for (u32 k = 0; k < 7; ++k) lds_sum(&hdr[GW_SUMS + k], sum[k]);
    lds_max(&kmax[1], key);
  }
  {  // the running nodes: the bits of upmap below N
    u64 c = 0;
    const u32 nw = (p.N + 31u) / 32u;
    for (u32 w = threadIdx.x; w < nw; w += BLOCK) {
      const u32 rest = p.N - w * 32u;
      c += (u32)__popc(p.upmap[w] & (rest >= 32u ? 0xFFFFFFFFu : (1u << rest) - 1u));
    }
    lds_sum(&hdr[GW_UP], c);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    hdr[GW_TICK] = p.now;
    hdr[GW_NODE_MAX] = kmax[0] >> 32;
    hdr[GW_NODE_ID] = kmax[0] ? 0xFFFFFFFFu - (u32)kmax[0] : 0u;
    hdr[GW_SUBJ_MAX] = kmax[1] >> 32;
    hdr[GW_SUBJ_ID] = kmax[1] ? 0xFFFFFFFFu - (u32)kmax[1] : 0u;
  }
  __syncthreads();
  if (threadIdx.x < SIM_GAZETTE_WORDS) p.out[threadIdx.x] = hdr[threadIdx.x];
}

__global__ void gazette_group_kernel(u32** grp, u32 g, u32* rows) { grp[g] = rows; }

// the ranking of a map's rows by a column (rank_candidates / rank_merge): every row is ranked, a row of zeros too
struct GazTopP {
  const u32* map;  // [N][8]
  u64 *ckey, *crec, *top;
  u32 N, G, top_k, column;
};
__global__ __launch_bounds__(BLOCK) void gazette_top_kernel(GazTopP p) {
  __shared__ u64 red[2][BLOCK / 64];
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;
  u64 w[GZ_RANK_WORDS] = {i, 0, 0, 0, 0}, key = 0;
  if (i < p.N) {
    const u64* row = reinterpret_cast<const u64*>(p.map + (size_t)i * SIM_GAZETTE_COLS);
#pragma unroll
    for (u32 k = 0; k < 4; ++k) w[1 + k] = row[k];
    const u32 v = p.map[(size_t)i * SIM_GAZETTE_COLS + p.column];
    key = (((u64)min(v, 0xFFFFFFFEu) << 32) | (u64)(0xFFFFFFFFu - i)) + 1ull;  // (never 0 = "none": a count of 0 is ranked; unique)
  }
  rank_candidates<GZ_RANK_WORDS>(key, w, p.ckey, p.crec, p.top_k, red);
}
__global__ __launch_bounds__(BLOCK) void gazette_top_fold(GazTopP p) {
  __shared__ u64 red[2][BLOCK / 64];
  rank_merge<GZ_RANK_WORDS>(p.ckey, p.crec, p.G, p.top_k, p.top, red, FillNoId());
}

// ---- host ----
struct GazetteState : Observer {  // samples of SIM_GAZETTE_WORDS words
  DevScratch<u32> d_nodes, d_subj;  // the maps, [N][8] each
  DevScratch<u32> d_shsub;          // [A]
  DevScratch<u32*> d_grp;           // [GZ_GROUPS]
  DevScratch<u64> d_hpart;          // [GZ_ROWS][G]
  DevScratch<u32> d_part, d_srec;   // [cap][8][G], [cap][8]
  std::vector<u32*> grp;            // the shadow's groups so far
  u32 G = 0, gslots = 1;
  u32 cap = 0;                      // slots the groups and the two arrays above have room for
  u32 range = 0;                    // the highest bound any sample has seen
  u32 window = 0;
  u64 expect = ~0ull;               // the handle's tick at which the next sample follows the last one (the start) without a gap
  ~GazetteState() override {
    for (u32* g : grp) (void)hipFree(g);
  }
  // room for slots 0 .. bound - 1: the shadow grows by whole groups as the high-water mark rises, the per-slot scratch with it
  int ensure(sim_handle* h, u32 bound) {
    if (bound <= cap) return SIM_OK;
    const Dev& d = h->d;
    HCHECK(hipStreamSynchronize(h->stream));  // (samples still enqueued use the scratch that is replaced)
    while ((u64)grp.size() * gslots < bound) {
      u32* g = nullptr;
      if (hipMalloc((void**)&g, std::max<size_t>((size_t)gslots * d.Nl, 1) * 4) != hipSuccess) { (void)hipGetLastError(); return SIM_ENOMEM; }
      grp.push_back(g);
      gazette_group_kernel<<<1, 1, 0, h->stream>>>(d_grp.get(), (u32)grp.size() - 1u, g);
    }
    const u32 ncap = (u32)std::min<u64>((u64)grp.size() * gslots, d.A);
    DevScratch<u32> np, ns;
    if (int rc = np.alloc((size_t)ncap * SIM_GAZETTE_COLS * G)) return rc;
    if (int rc = ns.alloc((size_t)ncap * SIM_GAZETTE_COLS)) return rc;
    d_part = std::move(np);
    d_srec = std::move(ns);
    cap = ncap;
    HCHECK(hipGetLastError());
    return SIM_OK;
  }
  int setup(sim_handle* h) {
    const Dev& d = h->d;
    G = (u32)std::min<size_t>(((size_t)d.Nl + BLOCK - 1) / BLOCK, GAZETTE_GRID);
    gslots = std::max(1u, (d.A + GZ_GROUPS - 1u) / GZ_GROUPS);
    const size_t map = (size_t)d.N * SIM_GAZETTE_COLS;
    if (int rc = d_nodes.alloc(map)) return rc;
    if (int rc = d_subj.alloc(map)) return rc;
    if (int rc = d_shsub.alloc(d.A)) return rc;
    if (int rc = d_grp.alloc(GZ_GROUPS)) return rc;
    if (int rc = d_hpart.alloc((size_t)GZ_ROWS * G)) return rc;
    HCHECK(hipMemsetAsync(d_nodes.get(), 0, map * 4, h->stream));
    HCHECK(hipMemsetAsync(d_subj.get(), 0, map * 4, h->stream));
    HCHECK(hipMemsetAsync(d_shsub.get(), 0xFF, std::max<size_t>(d.A, 1) * 4, h->stream));  // NOSLOT
    return launch(h, nullptr, true);  // the shadow of the state the handle is in
  }
  // behind the tick that was enqueued last: the diff against the shadow (rebase: the shadow re-taken instead), the sample into out (null: none)
  int launch(sim_handle* h, u64* out, bool rebase) {
    const Dev& d = h->d;
    const u32 bound = std::min(h->n_slots, d.A);
    if (int rc = ensure(h, bound)) return rc;
    range = std::max(range, bound);
    GazDevP p;
    p.view = d.view; p.subject_of = d.subject_of; p.upmap = d.upmap; p.base = h->d_base;
    p.grp = d_grp.get(); p.shsub = d_shsub.get(); p.nodes = d_nodes.get(); p.subj = d_subj.get();
    p.part = d_part.get(); p.hpart = d_hpart.get(); p.srec = d_srec.get(); p.out = out;
    p.N = d.N; p.Nl = d.Nl; p.G = G;
    p.bound = bound; p.range = range; p.gslots = gslots;
    p.now = (u32)h->tick; p.t = p.now - 1u;
    p.window = window;
    p.rebase = rebase ? 1u : 0u;
    if (rebase) {
      if (bound) gazette_shadow_kernel<<<G, BLOCK, 0, h->stream>>>(p);
    } else {
      gazette_scan_kernel<<<G, BLOCK, 0, h->stream>>>(p);  // (with no slot at all it still leaves its rows: zeros)
    }
    if (range) gazette_fold_kernel<<<(range + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
    if (out) gazette_pack_kernel<<<1, BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  }
  int sample(sim_handle* h, u64* out) override {
    if (int rc = launch(h, out, h->tick != expect)) return rc;
    expect = h->tick + smp.period;
    return SIM_OK;
  }
};
static inline GazetteState* gazette_of(const sim_handle* h) { return static_cast<GazetteState*>(h->obs[OB_GAZETTE]); }

// rows first .. first + n - 1 of a map
static int gazette_rows(sim_handle* h, bool subjects, u32 first, u32 n, sim_gazette_row* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out) return SIM_EINVAL;
  const GazetteState* s = gazette_of(h);
  if (!s) return SIM_ESTATE;
  if ((u64)first + n > h->d.N) return SIM_EINVAL;
  HCHECK(hipStreamSynchronize(h->stream));
  const u32* map = subjects ? s->d_subj.get() : s->d_nodes.get();
  if (n) HCHECK(hipMemcpy(out, map + (size_t)first * SIM_GAZETTE_COLS, (size_t)n * sizeof *out, hipMemcpyDeviceToHost));
  return SIM_OK;
}

extern "C" {

uint32_t sim_gazette_version(void) { return SIM_GAZETTE_VERSION; }

int sim_gazette_start(sim_handle* h, uint32_t first_tick, uint32_t period, uint32_t capacity, uint32_t flap_window) {
  GazetteState* s = new GazetteState();
  s->window = flap_window;
  const int rc = observer_start(h, OB_GAZETTE, s, SIM_GAZETTE_MAX_SAMPLES, first_tick, period, capacity, SIM_GAZETTE_WORDS,
                                [&] { return flap_window < SIM_INTERVAL_LIMIT ? SIM_OK : SIM_EINVAL; }, [&] { return s->setup(h); });
  if (rc == SIM_OK) s->expect = s->smp.first + 1;  // (the first sample follows the start's shadow)
  return rc;
}

int sim_gazette_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_GAZETTE, taken, dropped); }

int sim_gazette_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_GAZETTE, first, n, out, cap_words, n_out);
}

int sim_gazette_stop(sim_handle* h) { return observer_stop(h, OB_GAZETTE); }

int sim_gazette_nodes(sim_handle* h, uint32_t first, uint32_t n, sim_gazette_row* out) { return gazette_rows(h, false, first, n, out); }

int sim_gazette_subjects(sim_handle* h, uint32_t first, uint32_t n, sim_gazette_row* out) { return gazette_rows(h, true, first, n, out); }

int sim_gazette_top(sim_handle* h, uint32_t map, uint32_t column, uint32_t k, sim_gazette_rank* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out || map > SIM_GAZETTE_MAP_SUBJECTS || column >= SIM_GAZETTE_COLS || !k || k > SIM_GAZETTE_TOP_MAX) return SIM_EINVAL;
  const GazetteState* s = gazette_of(h);
  if (!s) return SIM_ESTATE;
  return observer_read_top(h, k, 1u, GZ_RANK_WORDS, out, [&](u64* ckey, u64* crec, u64* d_top, u32 G) -> int {
    GazTopP p;
    p.map = map == SIM_GAZETTE_MAP_SUBJECTS ? s->d_subj.get() : s->d_nodes.get();
    p.ckey = ckey; p.crec = crec; p.top = d_top;
    p.N = h->d.N; p.G = G; p.top_k = k; p.column = column;
    gazette_top_kernel<<<G, BLOCK, 0, h->stream>>>(p);
    gazette_top_fold<<<1, BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
}

}  // extern "C"
