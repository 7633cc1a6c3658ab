// serf_sim_observe.inc — part of the translation unit serf_sim.hip (included from there, behind the tick kernel; not a header of its own).
// What the observers of the simulated cluster share on the device — convergence, cluster stats and digests (serf_sim_kernels.inc), trackers,
// series, census, roll: wave reductions, the fold of a row of per-workgroup partial results, "has node l applied this rumour?".  Their shared
// host part (observer_usable, Sampler) needs the handle: end of serf_sim_host.inc.  Nothing the tick kernel uses is here.

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
