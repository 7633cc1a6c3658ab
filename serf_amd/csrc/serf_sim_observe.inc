// serf_sim_observe.inc — part of the translation unit serf_sim.hip (included from there, behind the tick kernel; not a header of its own).
// What the observers of the simulated cluster share on the device — convergence, cluster stats and digests (serf_sim_kernels.inc), trackers,
// series, census, roll, ledger, spread map, traffic meter, rumour tree:
//   wave reductions, the fold of a row of per-workgroup partial results, the workgroup's sum / max through LDS (lds_sum, lds_max), the
//   staging of a table in LDS (lds_stage);
//   "has node l applied this rumour?" (view_applied, bucket_holds, and rumour_held over both);
//   the ranking in two levels (group_max, rank_candidates, rank_merge) for one-word and two-word keys;
//   the walk over the packets a node sent last tick (sent_packets) and over the packets addressed to it (recv_packets), with the
//   Flight that says where those packets lie.
// Their shared host part (observer_usable, Sampler, the Observer frame, flight_fill, the tails of the reads) needs the handle: end of
// serf_sim_host.inc.  Nothing the tick kernel uses is here.

// ---- a value per lane -> the wave's sum / min / max, in every lane ----
__device__ static inline u64 wave_sum(u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ static inline u64 wave_min(u64 v) {
  for (int o = 32; o > 0; o >>= 1) { const u64 y = __shfl_xor(v, o); v = y < v ? y : v; }
  return v;
}
__device__ static inline u64 wave_max(u64 v) {
  for (int o = 32; o > 0; o >>= 1) { const u64 y = __shfl_xor(v, o); v = y > v ? y : v; }
  return v;
}

// ---- one wave combines the G partial results of one row (a workgroup's each: no atomics on global memory, nothing to zero) ----
enum { FOLD_SUM = 0, FOLD_MIN = 1, FOLD_MAX = 2 };
template <class T>
__device__ static inline u64 fold_row(const T* row, u32 G, u32 op) {
  u64 v = op == FOLD_MIN ? ~0ull : 0ull;
  for (u32 g = threadIdx.x & 63; g < G; g += 64) {
    const u64 y = row[g];
    v = op == FOLD_SUM ? v + y : op == FOLD_MIN ? (y < v ? y : v) : (y > v ? y : v);
  }
  return op == FOLD_SUM ? wave_sum(v) : op == FOLD_MIN ? wave_min(v) : wave_max(v);
}

// ---- has a node applied rumour (kind, key, ltime)? ----
// JOIN / LEAVE about a subject: `head` = the node's view entry of it (the default entry base[2 * subject] while it has no slot)
__device__ __forceinline__ static bool view_applied(uint4 head, u64 ltime) { return (head.w & SIM_VB_KNOWN) && E_LTIME(head) >= ltime; }
// EVENT / QUERY: bucket idx of `ring` (Dev::ering / qring, tail plane `tail` entries on), `head` = its head as the caller loaded it.
// Keys fill a bucket in order — head {ltime, k0, k1}, tail {k2 .. k5}, then its overflow rows (bucket_add) — and none is ever taken out:
// the tail is read only behind a full head, the overflow rows only behind a full tail — and not for key 0, "an empty place", where their walk ends.
__device__ __forceinline__ static bool bucket_holds(const Dev& d, const uint4* ring, size_t tail, u32 idx, size_t l, uint4 head, u32 key) {
  bool hit = (head.z == key) | (head.w == key);
  if (!hit && head.w) {
    const uint4 b1 = ring[(size_t)idx * d.Nl + l + tail];
    hit = (b1.x == key) | (b1.y == key) | (b1.z == key) | (b1.w == key);
    if (!hit && b1.w && key) hit = ovf_has(d, ring, tail, (u32)l, idx, key);
  }
  return hit;
}
// has node l (running) applied the rumour (kind, key, ltime)?  The predicate as convergence_many_kernel uses it, for one node
__device__ __forceinline__ static bool rumour_held(const Dev& d, const uint4* base, size_t l, u32 kind, u32 key, u64 ltime) {
  if (kind == SIM_K_JOIN || kind == SIM_K_LEAVE) {
    const u32 a = d.slot_of[key];
    const uint4 e = a == NOSLOT ? base[(size_t)key * 2] : d.view[(size_t)a * d.Nl + l];
    return view_applied(e, ltime);
  }
  const uint4* ring = kind == SIM_K_EVENT ? d.ering : d.qring;
  const u32 idx = (u32)(ltime % (kind == SIM_K_EVENT ? d.Bev : d.Bq));
  return bucket_holds(d, ring, kind == SIM_K_EVENT ? d.etail : d.qtail, idx, l, ring[(size_t)idx * d.Nl + l], key);
}

// ---- a workgroup's pieces ----
// a table (the entries an observer follows, uploaded once) staged in LDS, word by word; the caller's barrier follows
template <class T>
__device__ static inline void lds_stage(T& tab, const T* src_tab) {
  static_assert(sizeof(T) % 4 == 0, "staged into LDS word by word");
  const u32* src = reinterpret_cast<const u32*>(src_tab);
  u32* dst = reinterpret_cast<u32*>(&tab);
  for (u32 i = threadIdx.x; i < sizeof(T) / 4; i += BLOCK) dst[i] = src[i];
}
// lane-wise sum / maximum over the workgroup into LDS (the wave's first, then one LDS atomic a wave)
__device__ static inline void lds_sum(unsigned long long* dst, u64 v) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}
__device__ static inline void lds_max(unsigned long long* dst, u64 v) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0 && v) atomicMax(dst, (unsigned long long)v);
}

// ---- the ranking in two levels: every workgroup lists its top_k candidates, one workgroup merges the lists ----
// A key is unique among the ranked, so round r is "the largest key below round r - 1's", which needs no marking.  Two key types: u64
// with 0 = none (the roll, the traffic meter, the rumour tree), and WideKey — two words, compared s first, s == 0 = none — for the spread
// map, whose score, count and id together need more than 64 bits.  A key lies in ckey as key_words words; a first word of 0 ends a list.
struct WideKey { u64 s, r; };
__device__ static inline bool key_less(u64 a, u64 b) { return a < b; }
__device__ static inline bool key_less(WideKey a, WideKey b) { return a.s < b.s || (a.s == b.s && a.r < b.r); }
__device__ static inline bool key_same(u64 a, u64 b) { return a == b; }
__device__ static inline bool key_same(WideKey a, WideKey b) { return a.s == b.s && a.r == b.r; }
__device__ static inline bool key_none(u64 k) { return !k; }
__device__ static inline bool key_none(WideKey k) { return !k.s; }
__device__ static inline u64 key_shfl_xor(u64 k, int o) { return __shfl_xor(k, o); }
__device__ static inline WideKey key_shfl_xor(WideKey k, int o) { return WideKey{__shfl_xor(k.s, o), __shfl_xor(k.r, o)}; }
__device__ static inline void key_load(const u64* at, u64& k) { k = at[0]; }
__device__ static inline void key_load(const u64* at, WideKey& k) { k.s = at[0]; k.r = k.s ? at[1] : 0ull; }
__device__ static inline void key_store(u64* at, u64 k) { at[0] = k; }
__device__ static inline void key_store(u64* at, WideKey k) { at[0] = k.s; at[1] = k.r; }
template <class K> struct KeyLim;
template <> struct KeyLim<u64> { enum { WORDS = 1 }; __device__ static u64 none() { return 0ull; } __device__ static u64 all() { return ~0ull; } };
template <> struct KeyLim<WideKey> {
  enum { WORDS = 2 };
  __device__ static WideKey none() { return WideKey{0ull, 0ull}; }
  __device__ static WideKey all() { return WideKey{~0ull, ~0ull}; }
};
// the workgroup's largest key; red: [2][BLOCK / 64], the halves taken in turn (one barrier a call: a wave that is two calls ahead has
// passed the barrier of the call in between, which every wave reaches only behind its reads of this one)
template <class K>
__device__ static inline K group_max(K v, K (*red)[BLOCK / 64], u32 turn) {
  for (int o = 32; o > 0; o >>= 1) { const K y = key_shfl_xor(v, o); if (key_less(v, y)) v = y; }
  if ((threadIdx.x & 63) == 0) red[turn & 1u][threadIdx.x >> 6] = v;
  __syncthreads();
  K m = KeyLim<K>::none();
#pragma unroll
  for (u32 q = 0; q < BLOCK / 64; ++q) { const K y = red[turn & 1u][q]; if (key_less(m, y)) m = y; }
  return m;
}
// The workgroup's candidates, descending, into its lists ckey[G][top_k] / crec[G][top_k][W]: this lane's key (none: not ranked) and the
// W words of its record.  A list shorter than top_k ends with a terminator.  Every lane of the workgroup calls it
template <u32 W, class K>
__device__ static inline void rank_candidates(K key, const u64 (&w)[W], u64* ckey, u64* crec, u32 top_k, K (*red)[BLOCK / 64]) {
  K prev = KeyLim<K>::all();
  u64* ck = ckey + (size_t)blockIdx.x * top_k * KeyLim<K>::WORDS;
  u32 r = 0;
  for (; r < top_k; ++r) {  // (the same in every lane)
    const K m = group_max(key_less(key, prev) ? key : KeyLim<K>::none(), red, r);
    if (key_none(m)) break;
    if (key_same(key, m)) {
      u64* dst = crec + ((size_t)blockIdx.x * top_k + r) * W;
      key_store(ck + (size_t)r * KeyLim<K>::WORDS, m);
#pragma unroll
      for (u32 k = 0; k < W; ++k) dst[k] = w[k];
    }
    prev = m;
  }
  if (r < top_k && threadIdx.x == 0) ck[(size_t)r * KeyLim<K>::WORDS] = 0;
}
// One workgroup: the same selection over the G lists (each sorted: the largest key of a list below the last one chosen is the first
// below it) into top[top_k][W]; word k of a place that stays unused becomes fill(k).  Returns the places used, the same in every lane
template <u32 W, class K, class Fill>
__device__ static inline u32 rank_merge(const u64* ckey, const u64* crec, u32 G, u32 top_k, u64* top, K (*red)[BLOCK / 64], Fill fill) {
  K prev = KeyLim<K>::all();
  u32 r = 0;
  for (; r < top_k; ++r) {  // (the same in every lane)
    K best = KeyLim<K>::none();
    size_t at = 0;
    for (u32 g = threadIdx.x; g < G; g += BLOCK) {
      const size_t base = (size_t)g * top_k;
      for (u32 j = 0; j < top_k; ++j) {
        K k;
        key_load(ckey + (base + j) * KeyLim<K>::WORDS, k);
        if (key_none(k)) break;
        if (key_less(k, prev)) {
          if (key_less(best, k)) { best = k; at = base + j; }
          break;
        }
      }
    }
    const K m = group_max(best, red, r);
    if (key_none(m)) break;
    if (key_same(best, m)) {  // (keys are unique: one lane)
      const u64* src = crec + at * W;
      u64* dst = top + (size_t)r * W;
#pragma unroll
      for (u32 k = 0; k < W; ++k) dst[k] = src[k];
    }
    prev = m;
  }
  for (u32 k = r * W + threadIdx.x; k < top_k * W; k += BLOCK) top[k] = fill(k % W);
  return r;
}
// the two fills in use: zeros (the roll, the spread map); id 0xFFFFFFFF, then zeros (the traffic meter, the rumour tree)
struct FillZero { __device__ u64 operator()(u32) const { return 0ull; } };
struct FillNoId { __device__ u64 operator()(u32 k) const { return k ? 0ull : 0xFFFFFFFFull; } };

// ---- the packets in flight between two ticks ----
// Where the packets of the tick that just ended lie, filled by the host (flight_fill, serf_sim_host.inc)
struct Flight {
  const u32* rcsr;  // kRandomNodes: the graph of that tick, [Nl + 1] / [rcap]; null when the observer reads no rows
  const u32* rsrc;  // entries sender * 4 + slot
  u32 rcap;
  u32 cur;          // parity of the cells that hold the packets (obox[cur] / omap[cur])
  u32 nslot;        // fan-out slots that carry packets: f (random fan-out), feff of the tick that sent them (bijection)
};
// The packets node l sent, where they lie.  Its map word (obox[cur] / omap[cur]) holds 8 bits a slot: first page << 2 | pages - 1, 0xFF
// for none, the whole word 0xFFFFFFFF for a node that sent nothing.  Slots that hold the same field share ONE packet: it is read once, at
// its first slot.  The visitor — it decides what is loaded and what is kept — gets, per slot k < nslot that has a packet, in slot order:
//   v.page(k, wgt, cell)  every page of a distinct packet, first at slot k, that wgt slots map to: a cell of three uint4 (keys, value
//                         low words, value high bits + meta; 64- or 48-byte cells), never beyond the node's fp cells
//   v.packet(k, wgt)      behind its pages
//   v.repeat(k, first)    slot k maps to the packet that slot first < k has already shown
// The slot loops are unrolled: a visitor may keep a value per slot in registers
template <class V>
__device__ __forceinline__ static void sent_packets(const Dev& d, u32 cur, u32 nslot, size_t l, V& v) {
  const u32 jw = d.rfan ? d.obox[cur][l * RF_CELL_U4 + 3u].x : d.omap[cur][l];  // slot -> cell of the packets this node sent
  if (jw == 0xFFFFFFFFu) return;
  const size_t cu4 = d.rfan ? RF_CELL_U4 : PK_U4;
  const auto field = [&](u32 k) { return (jw >> (8u * k)) & 0xFFu; };
#pragma unroll
  for (u32 k = 0; k < SIM_MAX_FANOUT; ++k) {
    const u32 jb = field(k);
    if (k >= nslot || jb == 0xFFu) continue;
    u32 wgt = 0;
    bool again = false;
#pragma unroll
    for (u32 q = 0; q < SIM_MAX_FANOUT; ++q) {
      const bool same = q < nslot && field(q) == jb;
      if (same && q < k && !again) { again = true; v.repeat(k, q); }  // (q is a constant here)
      wgt += same ? 1u : 0u;
    }
    if (again) continue;
    const u32 np = min(jb & 3u, d.PG - 1u);
    for (u32 pg = 0; pg <= np && (jb >> 2) + pg < d.fp; ++pg)  // (never beyond the node's fp cells)
      v.page(k, wgt, d.obox[cur] + ((size_t)((jb >> 2) + pg) * d.Nl + l) * cu4);
    v.packet(k, wgt);
  }
}
// The packets addressed to node l: take(sender, slot) for each.  kRandomNodes: the row rsrc[rcsr[l] .. rcsr[l + 1]) of the graph of the
// tick that sent them; the bijection: the nslot sources through fan_source_g (ptp: that tick's parameters, unused under kRandomNodes)
template <class Take>
__device__ __forceinline__ static void recv_packets(const Dev& d, const TickP& ptp, const Flight& f, size_t l, Take take) {
  if (d.rfan) {
    const u32 b = f.rcsr[l], e = min(f.rcsr[l + 1], f.rcap);
    for (u32 i = b; i < e; ++i) {
      const u32 ent = f.rsrc[i];  // sender * 4 + slot
      if ((ent >> 2) < d.Nl) take(ent >> 2, ent & 3u);
    }
  } else {
    const u32 h = (u32)l / ptp.M, t = (u32)l - h * ptp.M;
#pragma unroll
    for (u32 k = 0; k < SIM_MAX_FANOUT; ++k) {
      if (k >= f.nslot) continue;
      u32 g, ll;
      fan_source_g(ptp, PICK4(ptp.off, k), PICK4(ptp.rot, k), PICK4(ptp.rho, k), h, t, k, g, ll);
      const u32 s = g * ptp.M + ll;
      if (s < d.Nl) take(s, k);
    }
  }
}
