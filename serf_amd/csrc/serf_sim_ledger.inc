// serf_sim_ledger.inc — part of the translation unit serf_sim.hip (included from there, after the roll; not a header of its own).
// Rumour ledger (include/serf_sim_ledger.h): three kernels behind a sampled tick's last launch, the host's bookkeeping, the entry points.
//
// Per sampled tick:
//   convergence_many_kernel  (serf_sim_kernels.inc, as it is) into scratch of the ledger's own: the reach of the entries of kinds 1-4 — the
//                        shared predicate (view_applied / bucket_holds, slot_of and the baseline) in the one place where it already
//                        stands.  Its counters are the only words that are zeroed beforehand (a memset of 8 + 8 n bytes on the stream)
//   ledger_count_kernel  a node per lane, grid-stride, LEDGER_GRID workgroups at most, whole waves kept together (the pass loop of
//                        series_sample_kernel).  The entries — uploaded at sim_ledger_start, not per sample — are staged once per
//                        workgroup in LDS next to an index by (kind, key): LEDGER_TAB buckets, a chain per bucket.  Every entry of a
//                        chain is compared: two entries may differ in val only.  A running node walks the groups of sort keys its
//                        count says are in use and the payload of each listed slot (the canonical record as canon_qrec assembles it:
//                        transmits from the key, kind from the payload's low byte); every node walks the packets it sent last tick
//                        (sent_packets, serf_sim_observe.inc), all three uint4 of every page of every distinct packet, weighted by the
//                        slots that map to it.  Hits are integer LDS adds into [n][LED_CNT] 32-bit counters;
//                        holders goes through a 64-bit mask per lane, once per node.  A workgroup sees Nl / LEDGER_GRID nodes — 16 Ki at
//                        the 16 Mi a handle can have — of SIM_Q = 64 records with 63 transmits at most: 2^26, far below 2^32; in flight
//                        a node sends fanout * pkt_records <= 2^7 record copies: 2^21.  The header's sums are wave reductions.  Every
//                        workgroup writes its column of a partial matrix [8 + LED_CNT n][G] as 64-bit words — no atomics on global
//                        memory, nothing to zero, the result does not depend on order.  A deep node (QDEEP, up to 64 entries through
//                        qused) and a multi-page packet (pkt_records 8 / 12 / 16) go through the same code
//   ledger_fold_kernel   one wave per word of the sample: folds its row (fold_row), or takes the entry's identity from the table, its
//                        reach from the reach pass's counters, and writes the word into the sample's slot
// Their order is the stream's.  The host knows every sampled tick in advance: it passes the slot to the launches and reads nothing back.
// A handle without a started ledger never gets here (sim_step_end finds its entry of the observers' table null).
#include "../../include/serf_sim_ledger.h"

static_assert(sizeof(sim_ledger_entry) == 16 && SIM_LEDGER_MAX == SIM_CONV_MAX && SIM_LEDGER_MAX == 64u && SIM_LEDGER_HEADER_WORDS == 8u &&
              SIM_LEDGER_ENTRY_WORDS == 8u, "layout of include/serf_sim_ledger.h; holders is a 64-bit mask; the reach pass takes every entry");

#define LEDGER_GRID 1024u  // workgroups of the count kernel at most
#define LEDGER_TAB 128u  // buckets of the LDS index by (kind, key)
#define LED_NONE 0xFFu     // end of a chain
#define LED_CNT 5u         // counters an entry: words LE_HOLD .. LE_FRESH
static_assert(LEDGER_TAB == 128u, "ledger_bucket keeps the top 7 bits");
// words of the header and of an entry (include/serf_sim_ledger.h)
enum { LH_TICK = 0, LH_UP = 1, LH_N = 2, LH_QUEUED = 3, LH_FLIGHT = 4, LH_PKTS = 5, LH_TX = 6 };
enum { LE_ID = 0, LE_VAL = 1, LE_REACH = 2, LE_HOLD = 3, LE_QUEUED = 4, LE_TX = 5, LE_FLIGHT = 6, LE_FRESH = 7 };
__host__ __device__ static inline u32 ledger_bucket(u32 kind, u32 key) { return (key * 0x9E3779B1u + kind * 0x85EBCA6Bu) >> 25; }
__host__ __device__ static inline bool ledger_has_row(u32 w) { return w == LH_UP || (w >= LH_QUEUED && w <= LH_TX); }

// the entries as the kernels read them: built and uploaded once, at sim_ledger_start / sim_ledger_now
struct LedTab {
  u64 id[SIM_LEDGER_MAX];        // key | kind << 32
  u64 val[SIM_LEDGER_MAX];
  u32 reach[SIM_LEDGER_MAX];     // 1 + the entry's place in the reach pass (ConvSet); 0: kinds 5-7, which have none
  uint8_t head[LEDGER_TAB];      // bucket -> its first entry, or LED_NONE
  uint8_t next[SIM_LEDGER_MAX];  // entry -> the next one of its chain, or LED_NONE
  u32 n, pad;
};

struct LedDevP {
  const LedTab* tab;
  const u64* reach;  // convergence_many_kernel's counters: [1 + i] nodes that have applied rumour i of the ConvSet
  u64* part;         // [8 + LED_CNT n][G]: every workgroup of the count kernel writes its column
  u64* out;          // the sample's slot: 8 + 8 n words
  u32 G;             // workgroups of the count kernel
  u32 n;             // entries
  u32 now;           // sim_tick after the sampled tick
  Flight fl;         // the packets in flight (cur and nslot: the ledger reads no rows)
};

// the entry a record (kind, key, val) matches, or LED_NONE; val: 64 bits of a queued record, 48 of one on the wire — SUSPECT / DEAD: the
// incarnation's 24 either way.  Entries are distinct: one matches at most
__device__ static inline u32 ledger_find(const LedTab& t, u32 kind, u32 key, u64 val) {
  const u64 id = (u64)key | ((u64)kind << 32);
  if (SIM_WIRE_TWO_PART(kind)) val &= 0xFFFFFFull;
  for (u32 e = t.head[ledger_bucket(kind, key)]; e < SIM_LEDGER_MAX; e = t.next[e])  // (LED_NONE ends it)
    if (t.id[e] == id && t.val[e] == val) return e;
  return LED_NONE;
}

__global__ __launch_bounds__(BLOCK) void ledger_count_kernel(Dev d, LedDevP p) {
  struct Sent {  // sent_packets' visitor: every record of a distinct packet weighs as many slots as map to it; a repeat slot adds nothing
    const LedTab& tab;
    u32* cnt;
    u32 &fl_all, &pkts;
    u32 any;
    __device__ void page(u32, u32 wgt, const uint4* cell) {
      const uint4 ck = ld4(cell), cl = ld4(cell + 1), ch = ld4(cell + 2);
      const u32 kw[4] = {ck.x, ck.y, ck.z, ck.w}, lw[4] = {cl.x, cl.y, cl.z, cl.w}, hw[4] = {ch.x, ch.y, ch.z, ch.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u32 kind = SIM_META_KIND(hw[r]) & 7u;
        if (!kind) continue;  // (an empty record is all zero)
        any = 1;
        fl_all += wgt;
        const u32 e = ledger_find(tab, kind, kw[r], (u64)lw[r] | ((u64)(hw[r] >> 16) << 32));
        if (e != LED_NONE) atomicAdd(&cnt[e * LED_CNT + (LE_FLIGHT - LE_HOLD)], wgt);  // (LDS)
      }
    }
    __device__ void packet(u32, u32 wgt) { pkts += any ? wgt : 0u; any = 0; }
    __device__ void repeat(u32, u32) {}
  };
  __shared__ LedTab tab;
  __shared__ u32 cnt[SIM_LEDGER_MAX * LED_CNT];
  __shared__ unsigned long long hdr[SIM_LEDGER_HEADER_WORDS];
  {
    lds_stage(tab, p.tab);
    for (u32 i = threadIdx.x; i < SIM_LEDGER_MAX * LED_CNT; i += BLOCK) cnt[i] = 0;
    if (threadIdx.x < SIM_LEDGER_HEADER_WORDS) hdr[threadIdx.x] = 0;
  }
  __syncthreads();
  u32 c_up = 0;                                       // a ballot per pass (the same value in every lane)
  u32 q_all = 0, tx_all = 0, fl_all = 0, pkts = 0;    // per lane, reduced over the wave once, at the end
  const size_t per_pass = (size_t)gridDim.x * BLOCK;
  const size_t passes = ((size_t)d.Nl + per_pass - 1) / per_pass;
  for (size_t it = 0; it < passes; ++it) {  // whole waves stay together: the ballot below needs every lane
    const size_t l = it * per_pass + (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool in = l < d.Nl;
    uint4 r1 = make_uint4(0, 0, 0, 0), r2 = r1;
    if (in) { r1 = ld4(&d.R1[l]); r2 = ld4(&d.R2[l]); }
    const bool up = in && (r1.z & SIM_RF_UP);
    c_up += (u32)__popcll(__ballot(up));
    // ---- the node's queue: keys ascending in groups of four, the records in the payload slots the keys name ----
    if (up) {
      const u32 depth = q_count(d, l, r2.z);
      u64 held = 0;
      for (u32 g = 0; 4u * g < depth; ++g) {
        const uint4 k4 = ld4(&d.qkeys[(size_t)g * d.Nl + l]);
        const u32 kk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
        for (u32 j = 0; j < 4; ++j) {
          if (4u * g + j >= depth) continue;
          const uint4 pay = ld4(&d.qpay[(size_t)(kk[j] & QK_SLOT_MASK) * d.Nl + l]);
          const u32 tx = (kk[j] >> QK_TX_SH) & 0x3Fu;  // SIM_META_TRANSMITS of the canonical record
          tx_all += tx;
          const u32 e = ledger_find(tab, SIM_META_KIND(pay.y), pay.x, (u64)pay.z | ((u64)pay.w << 32));
          if (e == LED_NONE) continue;
          atomicAdd(&cnt[e * LED_CNT + (LE_QUEUED - LE_HOLD)], 1u);  // (LDS)
          if (tx) atomicAdd(&cnt[e * LED_CNT + (LE_TX - LE_HOLD)], tx);
          else atomicAdd(&cnt[e * LED_CNT + (LE_FRESH - LE_HOLD)], 1u);
          held |= 1ull << e;
        }
      }
      q_all += depth;
      while (held) {  // once per node and entry, however many of its records match
        const u32 e = (u32)__ffsll((unsigned long long)held) - 1u;
        held &= held - 1ull;
        atomicAdd(&cnt[e * LED_CNT], 1u);
      }
    }
    // ---- the packets this node sent last tick, where they lie: a distinct packet weighs as many slots as map to it ----
    if (in) {
      Sent v = {tab, cnt, fl_all, pkts, 0u};
      sent_packets(d, p.fl.cur, p.fl.nslot, l, v);
    }
  }
  // ---- the workgroup's column ----
  {
    const bool lane0 = (threadIdx.x & 63) == 0;
    const u64 s[4] = {q_all, fl_all, pkts, tx_all};
    const u32 sw[4] = {LH_QUEUED, LH_FLIGHT, LH_PKTS, LH_TX};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u64 v = wave_sum(s[i]);
      if (lane0 && v) atomicAdd(&hdr[sw[i]], (unsigned long long)v);
    }
    if (lane0 && c_up) atomicAdd(&hdr[LH_UP], (unsigned long long)c_up);
  }
  __syncthreads();
  for (u32 w = threadIdx.x; w < SIM_LEDGER_HEADER_WORDS + LED_CNT * p.n; w += BLOCK)
    if (w >= SIM_LEDGER_HEADER_WORDS || ledger_has_row(w))
      p.part[(size_t)w * p.G + blockIdx.x] = w < SIM_LEDGER_HEADER_WORDS ? (u64)hdr[w] : (u64)cnt[w - SIM_LEDGER_HEADER_WORDS];
}

// one wave per word of the sample: its row of the partial matrix added up, or the entry's identity / reach; written into the sample's slot
__global__ __launch_bounds__(BLOCK) void ledger_fold_kernel(LedDevP p) {
  const u32 w = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= SIM_LEDGER_HEADER_WORDS + SIM_LEDGER_ENTRY_WORDS * p.n) return;  // (whole waves)
  u64 v = 0;
  if (w < SIM_LEDGER_HEADER_WORDS) {
    if (w == LH_TICK) v = p.now;
    else if (w == LH_N) v = p.n;
    else if (ledger_has_row(w)) v = fold_row(p.part + (size_t)w * p.G, p.G, FOLD_SUM);
  } else {
    const u32 i = (w - SIM_LEDGER_HEADER_WORDS) / SIM_LEDGER_ENTRY_WORDS, c = (w - SIM_LEDGER_HEADER_WORDS) % SIM_LEDGER_ENTRY_WORDS;
    if (c == LE_ID) v = p.tab->id[i];
    else if (c == LE_VAL) v = p.tab->val[i];
    else if (c == LE_REACH) { const u32 r = p.tab->reach[i]; v = r ? p.reach[r] : 0ull; }
    else v = fold_row(p.part + (size_t)(SIM_LEDGER_HEADER_WORDS + i * LED_CNT + (c - LE_HOLD)) * p.G, p.G, FOLD_SUM);
  }
  if (!lane) p.out[w] = v;
}

// ---- host ----
// what the kernels need besides the sample's place, for a given list of entries
struct LedScratch {
  DevScratch<LedTab> d_tab;
  DevScratch<u64> d_part;   // [8 + LED_CNT n][LEDGER_GRID]
  DevScratch<u64> d_reach;  // [1 + SIM_CONV_MAX]: convergence_many_kernel's counters
  ConvSet cs;               // the entries of kinds 1-4, as the reach pass takes them
  u32 n = 0;
};
static inline size_t ledger_stride(u32 n) { return SIM_LEDGER_HEADER_WORDS + (size_t)n * SIM_LEDGER_ENTRY_WORDS; }  // words of a sample

// the entries checked and put into the kernels' form; touches nothing but t and cs
static int ledger_check(const sim_handle* h, const sim_ledger_entry* e, u32 n, LedTab& t, ConvSet& cs) {
  if (!e || !n || n > SIM_LEDGER_MAX) return SIM_EINVAL;
  memset(&t, 0, sizeof t);
  memset(&cs, 0, sizeof cs);
  memset(t.head, LED_NONE, sizeof t.head);
  memset(t.next, LED_NONE, sizeof t.next);
  t.n = n;
  for (u32 i = 0; i < n; ++i) {
    const u32 kind = e[i].kind, key = e[i].key;
    const u64 val = e[i].val;
    if (kind < SIM_K_JOIN || kind > SIM_K_DEAD) return SIM_EINVAL;
    const bool named = kind == SIM_K_EVENT || kind == SIM_K_QUERY;  // the key is a name, not a subject
    if (named ? key == 0 : key >= h->d.N) return SIM_EINVAL;
    if (kind <= SIM_K_QUERY && val >> 48) return SIM_EINVAL;
    if (SIM_WIRE_TWO_PART(kind) && val >> 24) return SIM_EINVAL;
    for (u32 j = 0; j < i; ++j)
      if (e[j].kind == kind && e[j].key == key && e[j].val == val) return SIM_EINVAL;
    t.id[i] = (u64)key | ((u64)kind << 32);
    t.val[i] = val;
    if (kind <= SIM_K_QUERY) {
      cs.kind[cs.n] = kind; cs.key[cs.n] = key; cs.ltime[cs.n] = val;
      t.reach[i] = ++cs.n;
    }
    // the end of its bucket's chain: the entries of a chain stay in the order they were given
    const u32 b = ledger_bucket(kind, key);
    if (t.head[b] == LED_NONE) t.head[b] = (uint8_t)i;
    else {
      u32 at = t.head[b];
      while (t.next[at] != LED_NONE) at = t.next[at];
      t.next[at] = (uint8_t)i;
    }
  }
  return SIM_OK;
}
// checks, then the ring planes the reach pass reads (the route sim_track_add takes), the scratch and the table's upload
static int ledger_prepare(sim_handle* h, const sim_ledger_entry* e, u32 n, LedScratch& s) {
  LedTab t;
  if (int rc = ledger_check(h, e, n, t, s.cs)) return rc;
  for (u32 i = 0; i < s.cs.n; ++i)
    if (int rc = conv_plane(h, s.cs.kind[i], s.cs.ltime[i])) return rc;
  s.n = n;
  if (int rc = s.d_tab.alloc(1)) return rc;
  if (int rc = s.d_part.alloc((SIM_LEDGER_HEADER_WORDS + (size_t)LED_CNT * n) * LEDGER_GRID)) return rc;
  if (int rc = s.d_reach.alloc(SIM_CONV_MAX + 1)) return rc;
  HCHECK(hipMemcpy(s.d_tab.get(), &t, sizeof t, hipMemcpyHostToDevice));
  return SIM_OK;
}
// one ledger sample of the state the stream will be in when it gets here, into out[ledger_stride(n)]
static int ledger_launch(sim_handle* h, const LedScratch& s, u64* out) {
  const Dev& d = h->d;
  LedDevP p;
  p.tab = s.d_tab.get();
  p.reach = s.d_reach.get();
  p.part = s.d_part.get();
  p.out = out;
  p.G = (u32)std::min<size_t>(((size_t)d.Nl + BLOCK - 1) / BLOCK, LEDGER_GRID);
  p.n = s.n;
  p.now = (u32)h->tick;
  if (int rc = flight_fill(h, false, p.fl)) return rc;
  if (s.cs.n) {
    HCHECK(hipMemsetAsync(s.d_reach.get(), 0, (size_t)(s.cs.n + 1) * 8, h->stream));
    convergence_many_kernel<<<grid_for(d.Nl), BLOCK, 0, h->stream>>>(d, h->d_base, s.cs, s.d_reach.get());
  }
  ledger_count_kernel<<<p.G, BLOCK, 0, h->stream>>>(d, p);
  const u32 words = (u32)ledger_stride(s.n);
  ledger_fold_kernel<<<(words + BLOCK / 64 - 1) / (BLOCK / 64), BLOCK, 0, h->stream>>>(p);
  HCHECK(hipGetLastError());
  return SIM_OK;
}
struct LedgerState : Observer {  // samples of 8 + 8 n words
  LedScratch scr;
  int sample(sim_handle* h, u64* out) override { return ledger_launch(h, scr, out); }
};

extern "C" {

uint32_t sim_ledger_version(void) { return SIM_LEDGER_VERSION; }

int sim_ledger_start(sim_handle* h, const sim_ledger_entry* e, uint32_t n, uint32_t first_tick, uint32_t period, uint32_t capacity) {
  LedgerState* s = new LedgerState();
  const auto check = [&] {
    LedTab t;
    ConvSet cs;
    return ledger_check(h, e, n, t, cs);
  };
  return observer_start(h, OB_LEDGER, s, SIM_LEDGER_MAX_SAMPLES, first_tick, period, capacity, ledger_stride(n), check,
                        [&] { return ledger_prepare(h, e, n, s->scr); });
}

int sim_ledger_count(const sim_handle* h, uint32_t* taken, uint32_t* dropped) { return observer_count(h, OB_LEDGER, taken, dropped); }

int sim_ledger_read(sim_handle* h, uint32_t first, uint32_t n, uint64_t* out, size_t cap_words, uint32_t* n_out) {
  return observer_read(h, OB_LEDGER, first, n, out, cap_words, n_out);
}

int sim_ledger_stop(sim_handle* h) { return observer_stop(h, OB_LEDGER); }

int sim_ledger_now(sim_handle* h, const sim_ledger_entry* e, uint32_t n, uint64_t* out) {
  if (int rc = observer_usable(h)) return rc;
  if (!out) return SIM_EINVAL;
  // scratch of its own: a running ledger's table and partial matrix are those of ITS entries, and its samples still enqueued use them
  LedScratch own;
  if (int rc = ledger_prepare(h, e, n, own)) return rc;
  return observer_now(h, ledger_stride(n), out, [&](u64* d_out) { return ledger_launch(h, own, d_out); });
}

}  // extern "C"
