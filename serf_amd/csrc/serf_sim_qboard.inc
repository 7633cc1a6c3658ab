// serf_sim_qboard.inc — part of the translation unit serf_sim.hip (included from there, behind the tree; not a header of its own).
// Query board (include/serf_sim_qboard.h): two kernels behind a sampled tick's last launch, the kernels of the board's reads, the host's
// bookkeeping, the entry points.  It reads what the tick already keeps — qtab, the filter records and tag classes behind it, qbits — and
// writes none of it.
//
// Per sampled tick:
//   qboard_count_kernel  a node per lane, grid-stride, QBOARD_GRID workgroups at most, whole waves kept together (the series' pass loop).
//                        The ids — uploaded at sim_qboard_start, not per sample — are staged once per workgroup in LDS (lds_stage), and
//                        behind them every entry's table entry and filter head (qb_stage).  A lane reads its node's running flag and
//                        tag-class byte once.  Per entry that owns its table entry the wave makes ONE ballot of "eligible" (running and
//                        query_should_process, the device function the tick itself uses).  The wave's 64 nodes are two consecutive words
//                        of each bitmap: lane e loads entry e's — guarded, see below; one round trip a turn for all entries — and every lane
//                        gets them by a shuffle; the counts are popcounts of ballot AND words, kept by lane e for entry e.  Five counts an
//                        entry (acks, responses, eligible, answered, responded; silent is eligible - answered) and the running nodes go
//                        through LDS — one add a wave and count — into the workgroup's column of a partial matrix
//                        [1 + QB_ROWS n][G] as 64-bit words — no atomics on global memory, nothing to zero, no order to depend on.
//                        THE GUARD: a bitmap has ceil(N / 32) words.  When that is odd the last wave's second word is not the bitmap's:
//                        it is the first word of the response bitmap (node 0's response would count as an ack) and, for table entry
//                        255's response bitmap, past the allocation.  A word at or beyond ceil(N / 32) is not loaded, and the bits of
//                        nodes at or above N are masked by the ballot of "the lane has a node".
//   qboard_fold_kernel   one workgroup: a wave per row of the partial matrix (fold_row), then a lane per entry — the table entry decides
//                        the state, the entry's persistent record on the device (the 16 words of its previous sample: state, origin,
//                        deadline, previous counts, latches) gives `new` and the latches and is replaced —, then the header.
// The reads (each behind a wait for the stream — observer_settle —, on scratch of its own, the board untouched):
//   qboard_nodes_kernel  a node per lane: its record over the entries that own their table entry (qb_node_record)
//   qboard_silent_kernel ONE workgroup walks the nodes in chunks of BLOCK and compacts in ascending id (spread_unreached_kernel's idiom)
//   qboard_top_kernel / qboard_top_fold   the same record, ranked in two levels (rank_candidates / rank_merge) by
//                        (silent + 1) << 32 | (0xFFFFFFFF - id)
// A handle without a started board never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_qboard.h"

static_assert(sizeof(sim_qboard_node) == 64 && SIM_QBOARD_MAX == 64u && SIM_QBOARD_HEADER_WORDS == 8u && SIM_QBOARD_ENTRY_WORDS == 16u &&
              SIM_QBOARD_NODE_WORDS == 8u, "layout of include/serf_sim_qboard.h");
static_assert(SIM_QBOARD_TOP_MAX <= BLOCK, "a workgroup has top_k candidates at most among its BLOCK nodes");
static_assert(SIM_QBOARD_MAX <= BLOCK, "a lane per entry stages the descriptors and folds the entries");
static_assert(BLOCK % 64 == 0 && SIM_QBOARD_MAX <= 64u, "a wave's 64 nodes are two whole words of a bitmap; a lane per entry keeps its words and counts");

#define QBOARD_GRID 1024u  // workgroups of the count kernel at most
#define QB_ROWS 5u         // rows of the partial matrix an entry: acks, responses, eligible, answered, responded
// words of the header, of an entry and of a node's record (include/serf_sim_qboard.h)
enum { QH_TICK = 0, QH_UP = 1, QH_N = 2, QH_OPEN = 3, QH_CLOSED = 4, QH_WAITING = 5, QH_DISPLACED = 6, QH_NEW = 7 };
enum { QE_ID = 0, QE_ORIGIN = 1, QE_DEADLINE = 2, QE_ACKS = 3, QE_RESPONSES = 4, QE_ELIGIBLE = 5, QE_ANSWERED = 6, QE_RESPONDED = 7, QE_SILENT = 8,
       QE_NEW_ACKS = 9, QE_NEW_RESPONSES = 10, QE_T_FIRST = 11, QE_T_HALF = 12, QE_T_90 = 13, QE_T_99 = 14, QE_T_ALL = 15 };
enum { QR_ACKS = 0, QR_RESPONSES = 1, QR_ELIGIBLE = 2, QR_ANSWERED = 3, QR_RESPONDED = 4 };

// the ids as the kernels read them: built and uploaded once, at sim_qboard_start
struct QbTab {
  u32 id[SIM_QBOARD_MAX];
  u32 n, pad;
};
// what the table says about the entries now: loaded once per workgroup behind the ids
struct QbDesc {
  uint4 t[SIM_QBOARD_MAX];   // the table entry id % SIM_QT: {id, origin, deadline, flags}
  uint4 fh[SIM_QBOARD_MAX];  // the head of the filter record behind it
};

struct QbDevP {
  const QbTab* tab;
  u64* part;  // [1 + QB_ROWS n][G]: every workgroup of the count kernel writes its column
  u64* rec;   // [n][16]: every entry's previous sample; null: a stateless sample (sim_qboard_now)
  u64* out;   // the sample's slot: 8 + 16 n words
  u32 G;      // workgroups of the count kernel
  u32 n;      // entries
  u32 now;    // sim_tick after the sampled tick
};

// ids and descriptors into LDS; the caller's barrier follows
__device__ static inline void qb_stage(const Dev& d, QbTab& tab, QbDesc& ds, const QbTab* src) {
  lds_stage(tab, src);
  __syncthreads();
  if (threadIdx.x < SIM_QBOARD_MAX) {
    const u32 id = threadIdx.x < tab.n ? tab.id[threadIdx.x] : 0u;
    const u32 j = id % SIM_QT;
    ds.t[threadIdx.x] = id ? d.qtab[j] : make_uint4(0, 0, 0, 0);
    ds.fh[threadIdx.x] = id ? QFILT(d)[(size_t)j * (SIM_QF_WORDS / 4)] : make_uint4(0, 0, 0, 0);
  }
}
// node l's bit of table entry j's ack (which 0) / response (which 1) bitmap (l < N)
__device__ __forceinline__ static bool qb_bit(const Dev& d, size_t words, u32 j, u32 which, u32 l) {
  return (d.qbits[((size_t)j * 2 + which) * words + (l >> 5)] >> (l & 31u)) & 1u;
}

__global__ __launch_bounds__(BLOCK) void qboard_count_kernel(Dev d, QbDevP p) {
  __shared__ QbTab tab;
  __shared__ QbDesc ds;
  __shared__ u32 cnt[1 + SIM_QBOARD_MAX * QB_ROWS];  // the running nodes, then QB_ROWS counts an entry
  qb_stage(d, tab, ds, p.tab);
  for (u32 i = threadIdx.x; i < 1u + SIM_QBOARD_MAX * QB_ROWS; i += BLOCK) cnt[i] = 0;
  __syncthreads();
  const u32 lane = threadIdx.x & 63;
  const size_t words = ((size_t)d.N + 31) / 32;  // of one bitmap
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  u32 acc[QB_ROWS] = {0, 0, 0, 0, 0};  // lane e: the wave's counts of entry e
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together: the ballots and shuffles below need every lane
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in = l < d.Nl;
    const bool up = in && (d.R1[l].z & SIM_RF_UP);
    const u32 tcls = in ? TAGCLASS(d)[l] : 0u;
    const u64 inm = __ballot(in), mu = __ballot(up);
    if (!inm) continue;  // (the same in every lane)
    if (!lane && mu) atomicAdd(&cnt[0], (u32)__popcll(mu));  // (LDS)
    const size_t w0 = (l - lane) >> 5;  // the wave's nodes l - lane .. l - lane + 63 are words w0, w0 + 1 of a bitmap
    // lane e fetches entry e's two words of both bitmaps — all of a turn's loads are in flight together, not one round trip an entry —
    // and none at or beyond ceil(N / 32), which is another bitmap's or nobody's
    u32 a0 = 0, a1 = 0, r0 = 0, r1 = 0;
    if (lane < p.n && ds.t[lane].x == tab.id[lane]) {
      const u32* bits = d.qbits + (size_t)(tab.id[lane] % SIM_QT) * 2 * words;
      if (w0 < words) { a0 = bits[w0]; r0 = bits[words + w0]; }
      if (w0 + 1 < words) { a1 = bits[w0 + 1]; r1 = bits[words + w0 + 1]; }
    }
    for (u32 e = 0; e < p.n; ++e) {
      const u32 id = tab.id[e];
      if (ds.t[e].x != id) continue;  // the id does not own its table entry (the same in every lane)
      const u64 ack = ((u64)(u32)__shfl((int)a0, (int)e) | ((u64)(u32)__shfl((int)a1, (int)e) << 32)) & inm;  // (inm: no bits of nodes at or above N)
      const u64 rsp = ((u64)(u32)__shfl((int)r0, (int)e) | ((u64)(u32)__shfl((int)r1, (int)e) << 32)) & inm;
      const u64 me = __ballot(up && query_should_process(d, (u32)l, id, ds.fh[e], tcls));  // eligible
      if (lane == e) {  // lane e keeps entry e's counts over the turns
        acc[QR_ACKS] += (u32)__popcll(ack);
        acc[QR_RESPONSES] += (u32)__popcll(rsp);
        acc[QR_ELIGIBLE] += (u32)__popcll(me);
        acc[QR_ANSWERED] += (u32)__popcll(me & ack);
        acc[QR_RESPONDED] += (u32)__popcll(me & rsp);
      }
    }
  }
  if (lane < p.n) {
#pragma unroll
    for (u32 k = 0; k < QB_ROWS; ++k)
      if (acc[k]) atomicAdd(&cnt[1u + lane * QB_ROWS + k], acc[k]);  // (LDS: one add a wave and count)
  }
  __syncthreads();
  for (u32 w = threadIdx.x; w < 1u + QB_ROWS * p.n; w += BLOCK) p.part[(size_t)w * p.G + blockIdx.x] = cnt[w];
}

// one workgroup: the rows folded, a lane per entry, the header; written into the sample's slot and, with a board, into the records
__global__ __launch_bounds__(BLOCK) void qboard_fold_kernel(Dev d, QbDevP p) {
  __shared__ u64 sum[1 + SIM_QBOARD_MAX * QB_ROWS];
  __shared__ u32 st[SIM_QBOARD_MAX];
  __shared__ u64 fresh[SIM_QBOARD_MAX];  // an entry's new acks plus new responses
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (u32 w = wave; w < 1u + QB_ROWS * p.n; w += BLOCK / 64) {  // a wave per row
    const u64 v = fold_row(p.part + (size_t)w * p.G, p.G, FOLD_SUM);
    if (!lane) sum[w] = v;
  }
  __syncthreads();
  const u32 e = threadIdx.x;
  if (e < p.n) {
    const u32 id = p.tab->id[e];
    const uint4 t = d.qtab[id % SIM_QT];
    u64* rec = p.rec ? p.rec + (size_t)e * SIM_QBOARD_ENTRY_WORDS : nullptr;
    u64 w[SIM_QBOARD_ENTRY_WORDS];
#pragma unroll
    for (u32 k = 0; k < SIM_QBOARD_ENTRY_WORDS; ++k) w[k] = rec ? rec[k] : 0ull;  // the previous sample's
    const u32 was = (u32)(w[QE_ID] >> 32);
    u32 state;
    if (t.x != id) {  // not the owner: waiting until it has owned once, displaced from then on — the counts go, origin, deadline and latches stay
      state = was == SIM_QBOARD_WAITING ? SIM_QBOARD_WAITING : SIM_QBOARD_DISPLACED;
#pragma unroll
      for (u32 k = QE_ACKS; k <= QE_NEW_RESPONSES; ++k) w[k] = 0;
    } else {
      const u64 origin = (u64)t.y | ((u64)t.w << 32), deadline = t.z;
      // another query under this id (or the id back behind a displacement): the entry starts afresh
      const bool again = was == SIM_QBOARD_WAITING || was == SIM_QBOARD_DISPLACED || w[QE_ORIGIN] != origin || w[QE_DEADLINE] != deadline;
      const u64 prev_acks = again ? 0ull : w[QE_ACKS], prev_responses = again ? 0ull : w[QE_RESPONSES];
      if (again) {
#pragma unroll
        for (u32 k = QE_T_FIRST; k <= QE_T_ALL; ++k) w[k] = 0;
      }
      const u64* s = sum + 1u + e * QB_ROWS;
      const u64 el = s[QR_ELIGIBLE], a = s[QR_ANSWERED];
      const bool open = p.now <= t.z;
      state = open ? SIM_QBOARD_OPEN : SIM_QBOARD_CLOSED;
      w[QE_ORIGIN] = origin; w[QE_DEADLINE] = deadline;
      w[QE_ACKS] = s[QR_ACKS]; w[QE_RESPONSES] = s[QR_RESPONSES];
      w[QE_ELIGIBLE] = el; w[QE_ANSWERED] = a; w[QE_RESPONDED] = s[QR_RESPONDED]; w[QE_SILENT] = el - a;
      w[QE_NEW_ACKS] = rec ? s[QR_ACKS] - prev_acks : 0ull;
      w[QE_NEW_RESPONSES] = rec ? s[QR_RESPONSES] - prev_responses : 0ull;
      if (rec && open && el) {  // the trackers' conditions (include/serf_sim_track.h), answered against eligible; set once
        if (!w[QE_T_FIRST] && a >= 1) w[QE_T_FIRST] = p.now;
        if (!w[QE_T_HALF] && 2 * a >= el) w[QE_T_HALF] = p.now;
        if (!w[QE_T_90] && 10 * a >= 9 * el) w[QE_T_90] = p.now;
        if (!w[QE_T_99] && 100 * a >= 99 * el) w[QE_T_99] = p.now;
        if (!w[QE_T_ALL] && a == el) w[QE_T_ALL] = p.now;
      }
    }
    w[QE_ID] = (u64)id | ((u64)state << 32);
    u64* out = p.out + SIM_QBOARD_HEADER_WORDS + (size_t)e * SIM_QBOARD_ENTRY_WORDS;
#pragma unroll
    for (u32 k = 0; k < SIM_QBOARD_ENTRY_WORDS; ++k) {
      out[k] = w[k];
      if (rec) rec[k] = w[k];
    }
    st[e] = state;
    fresh[e] = w[QE_NEW_ACKS] + w[QE_NEW_RESPONSES];
  }
  __syncthreads();
  if (threadIdx.x < SIM_QBOARD_HEADER_WORDS) {  // a lane per word of the header
    const u32 c = threadIdx.x;
    u64 v = 0;
    if (c == QH_TICK) v = p.now;
    else if (c == QH_UP) v = sum[0];
    else if (c == QH_N) v = p.n;
    else if (c == QH_NEW) { for (u32 i = 0; i < p.n; ++i) v += fresh[i]; }
    else {
      const u32 want = c == QH_OPEN ? SIM_QBOARD_OPEN : c == QH_CLOSED ? SIM_QBOARD_CLOSED : c == QH_WAITING ? SIM_QBOARD_WAITING : SIM_QBOARD_DISPLACED;
      for (u32 i = 0; i < p.n; ++i) v += st[i] == want ? 1u : 0u;
    }
    p.out[c] = v;
  }
}

// ---- the reads of the board ----
// node i's record over the entries that own their table entry (`in`: the lane has a node)
__device__ static inline void qb_node_record(const Dev& d, const QbTab& tab, const QbDesc& ds, u32 i, bool in, bool up, u64 (&w)[SIM_QBOARD_NODE_WORDS]) {
  const size_t words = ((size_t)d.N + 31) / 32;
  const u32 tcls = in ? TAGCLASS(d)[i] : 0u;
  u32 asked = 0, acked = 0, responded = 0, silent_ack = 0, silent_resp = 0;
  for (u32 e = 0; e < tab.n; ++e) {
    const u32 id = tab.id[e];
    const uint4 t = ds.t[e];
    if (t.x != id || !in) continue;
    const bool ab = qb_bit(d, words, id % SIM_QT, 0, i), rb = qb_bit(d, words, id % SIM_QT, 1, i);
    const bool adm = query_should_process(d, i, id, ds.fh[e], tcls);
    asked += adm ? 1u : 0u;
    acked += ab ? 1u : 0u;
    responded += rb ? 1u : 0u;
    silent_ack += adm && (t.w & SIM_F_ACK) && !ab ? 1u : 0u;
    silent_resp += adm && (t.w & SIM_F_RESPOND) && !rb ? 1u : 0u;
  }
  w[0] = (u64)i | ((u64)(up ? 1u : 0u) << 32);
  w[1] = asked; w[2] = acked; w[3] = responded; w[4] = silent_ack; w[5] = silent_resp; w[6] = 0; w[7] = 0;
}

// the records of nodes first .. first + count - 1
__global__ __launch_bounds__(BLOCK) void qboard_nodes_kernel(Dev d, const QbTab* src, u32 first, u32 count, u64* out) {
  __shared__ QbTab tab;
  __shared__ QbDesc ds;
  qb_stage(d, tab, ds, src);
  __syncthreads();
  const u32 k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count) return;
  const u32 i = first + k;
  u64 w[SIM_QBOARD_NODE_WORDS];
  qb_node_record(d, tab, ds, i, true, d.R1[i].z & SIM_RF_UP, w);
  u64* dst = out + (size_t)k * SIM_QBOARD_NODE_WORDS;
#pragma unroll
  for (u32 q = 0; q < SIM_QBOARD_NODE_WORDS; ++q) dst[q] = w[q];
}

// the eligible nodes of query `id` without the bit `which`, ascending: ids[0 .. min(cap, total) - 1], *total; none when the id does not own its entry
__global__ __launch_bounds__(BLOCK) void qboard_silent_kernel(Dev d, u32 id, u32 which, u32* ids, u32 cap, u32* total) {
  __shared__ u32 wcnt[BLOCK / 64];
  const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 j = id % SIM_QT;
  const uint4 t = d.qtab[j], fh = QFILT(d)[(size_t)j * (SIM_QF_WORDS / 4)];
  const size_t words = ((size_t)d.N + 31) / 32;
  const size_t Nl = t.x == id ? (size_t)d.Nl : 0;  // (the same in every lane)
  u32 base = 0;  // the silent of the chunks before
  for (size_t l0 = 0; l0 < Nl; l0 += BLOCK) {  // (whole workgroups stay together: the barriers below)
    const size_t l = l0 + threadIdx.x;
    const bool un = l < Nl && (d.R1[l].z & SIM_RF_UP) && query_should_process(d, (u32)l, id, fh, TAGCLASS(d)[l]) && !qb_bit(d, words, j, which, (u32)l);
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

struct QbTopP {
  const QbTab* tab;
  u64* ckey;   // [G][top_k]: a workgroup's candidates, descending: (silent + 1) << 32 | (0xFFFFFFFF - id); 0 ends a shorter list
  u64* crec;   // [G][top_k][SIM_QBOARD_NODE_WORDS]: their records
  u64* nodes;  // null, or [Nl][SIM_QBOARD_NODE_WORDS]
  u64* top;    // [top_k][SIM_QBOARD_NODE_WORDS]
  u32 G;       // workgroups of the top kernel: ceil(Nl / BLOCK)
  u32 top_k, rank_by;
};
__global__ __launch_bounds__(BLOCK) void qboard_top_kernel(Dev d, QbTopP p) {
  __shared__ QbTab tab;
  __shared__ QbDesc ds;
  __shared__ u64 red[2][BLOCK / 64];
  qb_stage(d, tab, ds, p.tab);
  __syncthreads();
  const u32 i = blockIdx.x * BLOCK + threadIdx.x;  // the node
  const bool in = i < d.Nl;
  const bool up = in && (d.R1[in ? i : 0u].z & SIM_RF_UP);
  u64 w[SIM_QBOARD_NODE_WORDS];
  qb_node_record(d, tab, ds, i, in, up, w);
  if (p.nodes && in) {
    u64* dst = p.nodes + (size_t)i * SIM_QBOARD_NODE_WORDS;
#pragma unroll
    for (u32 k = 0; k < SIM_QBOARD_NODE_WORDS; ++k) dst[k] = w[k];
  }
  // the key: unique among the running nodes (0 for a node that does not run: never listed)
  const u64 key = up ? ((w[p.rank_by == SIM_QBOARD_BY_SILENT_ACK ? 4 : 5] + 1ull) << 32) | (u64)(0xFFFFFFFFu - i) : 0ull;
  rank_candidates<SIM_QBOARD_NODE_WORDS>(key, w, p.ckey, p.crec, p.top_k, red);
}
// one workgroup: the lists merged; writes the listed records, zeroing what stays unused
__global__ __launch_bounds__(BLOCK) void qboard_top_fold(QbTopP p) {
  __shared__ u64 red[2][BLOCK / 64];
  rank_merge<SIM_QBOARD_NODE_WORDS>(p.ckey, p.crec, p.G, p.top_k, p.top, red, FillZero());
}

// ---- host ----
static inline size_t qboard_stride(u32 n) { return SIM_QBOARD_HEADER_WORDS + (size_t)n * SIM_QBOARD_ENTRY_WORDS; }  // words of a sample
static inline u32 qboard_grid(const sim_handle* h) { return (u32)std::min<size_t>(((size_t)h->d.Nl + BLOCK - 1) / BLOCK, QBOARD_GRID); }

// the ids checked and put into the kernels' form; touches nothing but t
static int qboard_check(const u32* ids, u32 n, QbTab& t) {
  if (!ids || !n || n > SIM_QBOARD_MAX) return SIM_EINVAL;
  memset(&t, 0, sizeof t);
  t.n = n;
  for (u32 i = 0; i < n; ++i) {
    if (!ids[i]) return SIM_EINVAL;
    for (u32 j = 0; j < i; ++j)
      if (ids[j] == ids[i]) return SIM_EINVAL;
    t.id[i] = ids[i];
  }
  return SIM_OK;
}

// what a sample's two launches need on the device: the ids and the partial matrix
struct QbScratch {
  DevScratch<QbTab> d_tab;
  DevScratch<u64> d_part;  // [1 + QB_ROWS n][QBOARD_GRID]
  QbTab t;                 // the host's copy of the ids
  u32 n = 0;
  int prepare(const u32* ids, u32 cnt) {
    if (int rc = qboard_check(ids, cnt, t)) return rc;
    n = cnt;
    if (int rc = d_tab.alloc(1)) return rc;
    if (int rc = d_part.alloc((1u + (size_t)QB_ROWS * n) * QBOARD_GRID)) return rc;
    HCHECK(hipMemcpy(d_tab.get(), &t, sizeof t, hipMemcpyHostToDevice));
    return SIM_OK;
  }
};
// one sample of the state the stream will be in when it gets here; rec: the board's records, or null for a stateless one
static int qboard_launch(sim_handle* h, const QbScratch& s, u64* rec, u64* out) {
  QbDevP p;
  p.tab = s.d_tab.get(); p.part = s.d_part.get(); p.rec = rec; p.out = out;
  p.G = qboard_grid(h);
  p.n = s.n;
  p.now = (u32)h->tick;
  qboard_count_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d, p);
  qboard_fold_kernel<<<1, BLOCK, 0, h->stream>>>(h->d, p);
  HCHECK(hipGetLastError());
  return SIM_OK;
}

struct QBoardState : Observer {  // samples of 8 + 16 n words
  QbScratch scr;
  DevScratch<u64> d_rec;  // [n][16]: every entry's previous sample (all zero: waiting)
  int setup(sim_handle* h, const u32* ids, u32 cnt) {
    if (int rc = scr.prepare(ids, cnt)) return rc;
    if (int rc = d_rec.alloc((size_t)cnt * SIM_QBOARD_ENTRY_WORDS)) return rc;
    HCHECK(hipMemsetAsync(d_rec.get(), 0, (size_t)cnt * SIM_QBOARD_ENTRY_WORDS * 8, h->stream));
    return SIM_OK;
  }
  int sample(sim_handle* h, u64* out) override { return qboard_launch(h, scr, d_rec.get(), out); }
};
static inline QBoardState* qboard_of(const sim_handle* h) { return static_cast<QBoardState*>(h->obs[OB_QBOARD]); }

extern "C" {

uint32_t sim_qboard_version(void) { return SIM_QBOARD_VERSION; }

int sim_qboard_start(sim_handle* h, const uint32_t* ids, uint32_t n, uint32_t first_tick, uint32_t period, uint32_t capacity) {
  QBoardState* s = new QBoardState();
  const auto check = [&] {
    QbTab t;
    return qboard_check(ids, n, t);
  };
  return observer_start(h, OB_QBOARD, s, SIM_QBOARD_MAX_SAMPLES, first_tick, period, capacity, qboard_stride(n), check,
                        [&] { return s->setup(h, ids, n); });
}

int sim_qboard_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_QBOARD, taken, dropped); }

int sim_qboard_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_QBOARD, first, n, out, cap_words, n_out);
}

int sim_qboard_stop(sim_handle* h) { return observer_stop(h, OB_QBOARD); }

int sim_qboard_now(sim_handle* h, const uint32_t* ids, uint32_t n, uint64_t* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out) return SIM_EINVAL;
  // scratch of its own: a running board's table and partial matrix are those of ITS ids, and its samples still enqueued use them
  QbScratch own;
  if (int rc = own.prepare(ids, n)) return rc;
  return observer_now(h, qboard_stride(n), out, [&](u64* d_out) { return qboard_launch(h, own, nullptr, d_out); });
}

int sim_qboard_silent(sim_handle* h, uint32_t entry, uint32_t which, uint32_t* ids, uint32_t cap, uint32_t* n_out, uint32_t* total) {
  if (int rc = observer_usable(h)) return rc;
  if (!n_out || !total || (cap && !ids) || which > 1u) return SIM_EINVAL;
  const QBoardState* s = qboard_of(h);
  if (!s) return SIM_ESTATE;
  if (entry >= s->scr.n) return SIM_EINVAL;
  const u32 id = s->scr.t.id[entry];
  return observer_read_ids(h, ids, cap, n_out, total, [&](u32* d_ids, u32 room, u32* d_total) -> int {
    qboard_silent_kernel<<<1, BLOCK, 0, h->stream>>>(h->d, id, which, d_ids, room, d_total);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
}

int sim_qboard_nodes(sim_handle* h, uint32_t first_node, uint32_t count, sim_qboard_node* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out) return SIM_EINVAL;
  const QBoardState* s = qboard_of(h);
  if (!s) return SIM_ESTATE;
  if ((u64)first_node + count > h->d.N) return SIM_EINVAL;
  DevScratch<u64> d_out;
  if (int rc = d_out.alloc((size_t)count * SIM_QBOARD_NODE_WORDS)) return rc;
  int rc = observer_settle(h, [&]() -> int {
    if (!count) return SIM_OK;
    qboard_nodes_kernel<<<(count + BLOCK - 1) / BLOCK, BLOCK, 0, h->stream>>>(h->d, s->scr.d_tab.get(), first_node, count, d_out.get());
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
  if (rc != SIM_OK) return rc;
  if (count) HCHECK(hipMemcpy(out, d_out.get(), (size_t)count * sizeof *out, hipMemcpyDeviceToHost));
  return SIM_OK;
}

int sim_qboard_top(sim_handle* h, uint32_t top_k, uint32_t rank_by, sim_qboard_node* top, sim_qboard_node* nodes) {
  if (int rc = observer_usable(h)) return rc;
  if (!top || !top_k || top_k > SIM_QBOARD_TOP_MAX || rank_by > SIM_QBOARD_BY_SILENT_RESP) return SIM_EINVAL;
  const QBoardState* s = qboard_of(h);
  if (!s) return SIM_ESTATE;
  DevScratch<u64> d_nodes;
  if (nodes)
    if (int rc = d_nodes.alloc((size_t)h->d.Nl * SIM_QBOARD_NODE_WORDS)) return rc;
  int rc = observer_read_top(h, top_k, 1u, SIM_QBOARD_NODE_WORDS, top, [&](u64* ckey, u64* crec, u64* d_top, u32 G) -> int {
    QbTopP p;
    p.tab = s->scr.d_tab.get(); p.ckey = ckey; p.crec = crec;
    p.nodes = nodes ? d_nodes.get() : nullptr;
    p.top = d_top;
    p.G = G;
    p.top_k = top_k; p.rank_by = rank_by;
    qboard_top_kernel<<<p.G, BLOCK, 0, h->stream>>>(h->d, p);
    qboard_top_fold<<<1, BLOCK, 0, h->stream>>>(p);
    HCHECK(hipGetLastError());
    return SIM_OK;
  });
  if (rc != SIM_OK) return rc;
  if (nodes) HCHECK(hipMemcpy(nodes, d_nodes.get(), (size_t)h->d.N * sizeof *nodes, hipMemcpyDeviceToHost));
  return SIM_OK;
}

}  // extern "C"
