// Routing of ECDSA lanes to the keyed verifier for gfx950 -- kernel K15.
//
// Part of ecdsa.hip's translation unit (included at its end, inside namespace
// cordahip, after ecdsa_vkey.hip): the field functions, the generic engine's lane
// bodies and K13's lane body are used as they are.
//
// With cordahip_vkey_set_routing_ecdsa on and a live ECDSA verification key on the
// device, every batch that reaches ec_verify_enqueue (runtime.cpp) is split on the
// GPU: lanes whose scheme and key bytes name a live record's point go to K13
// (ecdsa_verify_keyed_idx_kernel, one instance per curve over that curve's run of
// perm, so a wave holds one curve only), the others to K2 (indexed instances of prep
// and ladder over the generic list). The match rule, the classes, the order in perm
// and the scratch layout are ecdsa_route.hpp. The host never reads a count back: the
// indexed kernels take their lane counts from the partition's counters.

// The live records' points as the bytes lanes carry: one thread per slot, gathered in
// slot order into the scratch header. Entry (j = 0, d = 1) of a key's table is the
// point itself (affine, canonical, Montgomery form).
template <class F>
CDEV void ec_route_plain(uint32_t w[8], const f29& m) {
  f29 p;
  f29_from_mont<F>(p, m);
  f29_to_words(w, p);
}

__global__ void __launch_bounds__(64) ecdsa_route_gather_kernel(const uint32_t* __restrict__ vtab,
                                                               uint32_t* __restrict__ scratch) {
  const uint32_t slot = threadIdx.x;
  const uint32_t* rec = vtab + kEcVkeyRecBase + slot * kEcVkeyRecWords;
  const bool live = slot < kVkeySlots && ec_route_rec_live(rec);
  const unsigned long long b = __ballot(live);
  if (live) {
    const uint32_t sch = rec[kEcVkeyRecScheme];
    f29 x, y;
    load_g(x, y, vtab + (size_t)slot * kEcVkeyTableWords + ec_vkey_entry_word(0, 1), 0);
    uint32_t xw[8], yw[8];
    if (sch == 2) {
      ec_route_plain<K1F>(xw, x);
      ec_route_plain<K1F>(yw, y);
    } else {
      ec_route_plain<R1F>(xw, x);
      ec_route_plain<R1F>(yw, y);
    }
    ec_route_put(scratch + kEcRouteRecBase, route_rank(b, slot), sch, rec[kEcVkeyRecId], xw, yw);
  }
  if (slot == 0) scratch[kEcRouteCntLive] = (uint32_t)__popcll(b);
}

// hdr: the scratch header the gather kernel filled; route: route[n] behind it.
// counts: the partition's seven class counts (zeroed by the launcher). totals: the
// device's cumulative keyed / generic lane counters. count (K24, the mixed device calls;
// null: every one of the n lanes): the rows to partition, known on the device only and
// clipped to n before anything is indexed; rows at or past it enter no class.
__global__ void __launch_bounds__(256) ecdsa_route_kernel(const uint8_t* __restrict__ scheme,
                                                         const uint8_t* __restrict__ keys,
                                                         const uint8_t* __restrict__ key_len, uint64_t n,
                                                         const uint32_t* __restrict__ hdr,
                                                         uint32_t* __restrict__ route,
                                                         unsigned int* __restrict__ counts,
                                                         unsigned long long* __restrict__ totals,
                                                         const uint32_t* __restrict__ count) {
  if (count) n = route_count_clip(*count, n);
  __shared__ uint32_t recs[kVkeySlots * kEcRouteRecWords];
  __shared__ unsigned int part[kEcRouteClasses][4];
  const uint32_t nlive = hdr[kEcRouteCntLive] < kVkeySlots ? hdr[kEcRouteCntLive] : kVkeySlots;
  for (uint32_t w = threadIdx.x; w < nlive * kEcRouteRecWords; w += 256) recs[w] = hdr[kEcRouteRecBase + w];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int tot[kEcRouteClasses] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll 1
  for (int it = 0; it < kEcRouteIter; it++) {
    const uint64_t i = ec_route_tile_lane(blockIdx.x, it, threadIdx.x);
    int c = -1;
    if (i < n) {
      const uint8_t sch = scheme[i], kl = key_len[i];
      const uint32_t id = ec_route_match(sch, kl, keys + i * 65, recs, nlive);
      route[i] = id;
      c = ec_route_class(sch, kl, id);
    }
#pragma unroll
    for (int k = 0; k < kEcRouteClasses; k++) tot[k] += (unsigned int)__popcll(__ballot(c == k));
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kEcRouteClasses; k++) part[k][wave] = tot[k];
  }
  __syncthreads();
  if (threadIdx.x < kEcRouteClasses) {
    const unsigned int t = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
    if (t) {
      atomicAdd(&counts[threadIdx.x], t);
      atomicAdd(&totals[threadIdx.x < kEcRouteGenericClasses ? 1 : 0], (unsigned long long)t);
    }
  }
}

// ecdsa_scatter_kernel with the class taken from route[i]: perm holds the seven
// classes' runs in order (ecdsa_route.hpp), one atomic per class per wave.
__global__ void __launch_bounds__(256) ecdsa_scatter_routed_kernel(const uint8_t* __restrict__ scheme,
                                                                  const uint8_t* __restrict__ key_len,
                                                                  const uint32_t* __restrict__ route, uint64_t n,
                                                                  const unsigned int* __restrict__ counts,
                                                                  unsigned int* __restrict__ cursors,
                                                                  unsigned int* __restrict__ perm,
                                                                  const uint32_t* __restrict__ count) {
  if (count) n = route_count_clip(*count, n);  // K24, as in the route kernel
  const int lane = threadIdx.x & 63;
  unsigned int tot[kEcRouteClasses] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll 4
  for (int it = 0; it < kEcRouteIter; it++) {
    const uint64_t i = ec_route_tile_lane(blockIdx.x, it, threadIdx.x);
    const int c = i < n ? ec_route_class(scheme[i], key_len[i], route[i]) : -1;
#pragma unroll
    for (int k = 0; k < kEcRouteClasses; k++) tot[k] += (unsigned int)__popcll(__ballot(c == k));
  }
  unsigned int start[kEcRouteClasses];
  unsigned int base = 0;
#pragma unroll
  for (int k = 0; k < kEcRouteClasses; k++) {
    unsigned int s0 = 0;
    if (lane == 0 && tot[k]) s0 = atomicAdd(&cursors[k], tot[k]);
    start[k] = __shfl(s0, 0) + base;
    base += counts[k];
  }
#pragma unroll 4
  for (int it = 0; it < kEcRouteIter; it++) {
    const uint64_t i = ec_route_tile_lane(blockIdx.x, it, threadIdx.x);
    const int c = i < n ? ec_route_class(scheme[i], key_len[i], route[i]) : -1;
#pragma unroll
    for (int k = 0; k < kEcRouteClasses; k++) {
      const unsigned long long m = __ballot(c == k);
      if (c == k) perm[start[k] + route_rank(m, (uint32_t)lane)] = (unsigned int)i;
      start[k] += (unsigned int)__popcll(m);
    }
  }
}

// K13 over one curve's keyed run of perm: thread j below the run's count takes lane
// perm[start + j], its key id from route[]. The grid covers every lane of the batch;
// blocks past the count exit at once. Messages as the generic engine has them:
// msg_off non-null: n + 1 CSR offsets; else dense rows of msg_len bytes.
template <int S>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) ecdsa_verify_keyed_idx_kernel(
    const uint32_t* __restrict__ route, const unsigned int* __restrict__ perm,
    const unsigned int* __restrict__ counts, const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ sig_len,
    const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ msg_off, uint32_t msg_len,
    const uint8_t* __restrict__ pre, uint32_t empty_is_error, const uint32_t* __restrict__ vtab,
    uint8_t* __restrict__ status) {
  const uint64_t cnt = ec_route_keyed_count(counts, S);
  if ((uint64_t)blockIdx.x * blockDim.x >= cnt) return;
  ec_verify_keyed_lane<S, true>(route, perm + ec_route_keyed_start(counts, S), sigs, sig_len, msgs, msg_off, nullptr,
                                msg_len, cnt, pre, empty_is_error, vtab, status);
}

// The generic engine's prep and ladder over the generic list perm[0 .. g) of a routed
// batch: the chunk at list position base holds route_chunk_lanes(g, base, m) records,
// g read from the counts; a chunk or a block wholly past it does nothing.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) ecdsa_prep_idx_kernel(
    const unsigned int* __restrict__ perm, const unsigned int* __restrict__ counts,
    const uint8_t* __restrict__ scheme, const uint8_t* __restrict__ keys, const uint8_t* __restrict__ key_len,
    const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ sig_len, const uint8_t* __restrict__ msgs,
    const uint64_t* __restrict__ msg_off, uint32_t msg_len, uint64_t base, uint64_t m,
    const uint8_t* __restrict__ pre_status, uint8_t* __restrict__ status, uint32_t* __restrict__ ws,
    uint32_t empty_is_error) {
  const uint64_t mm = route_chunk_lanes(ec_route_generic_count(counts), base, m);
  if ((uint64_t)blockIdx.x * blockDim.x >= mm) return;
  ecdsa_prep_body<true>(perm, scheme, keys, key_len, sigs, sig_len, msgs, msg_off, msg_len, base, mm, pre_status,
                        status, ws, empty_is_error);
}

template <int S>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) ecdsa_ladder_idx_kernel(
    const unsigned int* __restrict__ perm, const unsigned int* __restrict__ counts,
    const uint8_t* __restrict__ scheme, uint64_t base, uint64_t m, const uint32_t* __restrict__ gtab,
    uint32_t* __restrict__ ws, uint8_t* __restrict__ status) {
  const uint64_t mm = route_chunk_lanes(ec_route_generic_count(counts), base, m);
  if ((uint64_t)blockIdx.x * blockDim.x >= mm) return;
  ecdsa_ladder_body<S, true>(perm, scheme, base, mm, gtab, ws, status);
}

// ---------------------------------------------------------------------------
// host-side launchers (called by runtime.cpp)

// what the runtime allocates for a batch of n lanes (a capacity: ecdsa_route.hpp)
size_t ecdsa_route_scratch_bytes(uint64_t n) {
  return (size_t)ec_route_scratch_words(route_scratch_cap_lanes(n)) * sizeof(uint32_t);
}
uint64_t ecdsa_route_max_lanes() { return kRouteMaxLanes; }

// gather, route, scatter: scratch (ecdsa_route_scratch_bytes(n)), counters (counts[7]
// and cursors[7], zeroed here) and perm[n] filled; totals += (keyed, generic)
hipError_t launch_ecdsa_route(const uint8_t* scheme, const uint8_t* keys, const uint8_t* key_len, uint64_t n,
                              const uint32_t* vtab, uint32_t* scratch, unsigned int* counters, unsigned int* perm,
                              unsigned long long* totals, hipStream_t s, const uint32_t* count) {
  if (n == 0 || n > kRouteMaxLanes || !vtab || !scratch || !counters || !perm || !totals) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counters, 0, 2 * kEcRouteClasses * sizeof(unsigned int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ecdsa_route_gather_kernel, dim3(1), dim3(64), 0, s, vtab, scratch);
  const dim3 pgrid((uint32_t)((n + kEcRouteTile - 1) / kEcRouteTile));
  hipLaunchKernelGGL(ecdsa_route_kernel, pgrid, dim3(256), 0, s, scheme, keys, key_len, n, scratch,
                     scratch + ec_route_off_route(), counters, totals, count);
  hipLaunchKernelGGL(ecdsa_scatter_routed_kernel, pgrid, dim3(256), 0, s, scheme, key_len,
                     scratch + ec_route_off_route(), n, counters, counters + kEcRouteClasses, perm, count);
  return hipGetLastError();
}

// K13 over the keyed runs of a routed batch of n lanes: the instance of every curve
// that has a live key (a curve without one has an empty run)
hipError_t launch_ecdsa_verify_keyed_idx(const uint32_t* scratch, const unsigned int* perm,
                                         const unsigned int* counters, uint64_t n, const uint8_t* sigs,
                                         const uint8_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off,
                                         uint32_t msg_len, const uint8_t* pre, uint32_t flags, const uint32_t* vtab,
                                         bool live_k1, bool live_r1, uint8_t* status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n > kRouteMaxLanes || !vtab) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)((n + 255) / 256));
  const uint32_t eie = (flags & 1u) ? 0u : 1u;
  const uint32_t* route = scratch + ec_route_off_route();
  if (live_k1)
    hipLaunchKernelGGL(ecdsa_verify_keyed_idx_kernel<2>, grid, dim3(256), 0, s, route, perm, counters, sigs, sig_len,
                       msgs, msg_off, msg_len, pre, eie, vtab, status);
  if (live_r1)
    hipLaunchKernelGGL(ecdsa_verify_keyed_idx_kernel<3>, grid, dim3(256), 0, s, route, perm, counters, sigs, sig_len,
                       msgs, msg_off, msg_len, pre, eie, vtab, status);
  return hipGetLastError();
}

// The generic engine over the generic list of a routed batch of n lanes: one prep /
// inversion / ladder set per ws_slots list positions. The host does not know the
// list's length, so the sets cover all n positions; a set wholly past the count does
// nothing (ecdsa_inv_kernel clips itself to the curve runs, which end at the count).
// Then the verdict words from the final statuses, as launch_ecdsa_verify.
hipError_t launch_ecdsa_verify_routed(const uint8_t* scheme, const uint8_t* keys, const uint8_t* key_len,
                                      const uint8_t* sigs, const uint8_t* sig_len, const uint8_t* msgs,
                                      const uint64_t* msg_off, uint32_t msg_len, uint64_t n, const uint32_t* gk1,
                                      const uint32_t* gr1, const uint8_t* pre_status, uint8_t* status,
                                      unsigned long long* verdict, const unsigned int* counters,
                                      const unsigned int* perm, uint32_t* ws, uint64_t ws_slots, uint32_t flags,
                                      hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (!ws || ws_slots < 64 || !counters || !perm) return hipErrorInvalidValue;
  for (uint64_t base = 0; base < n; base += ws_slots) {
    const uint64_t m = n - base < ws_slots ? n - base : ws_slots;
    const dim3 g((uint32_t)((m + 255) / 256));
    hipLaunchKernelGGL(ecdsa_prep_idx_kernel, g, dim3(256), 0, s, perm, counters, scheme, keys, key_len, sigs, sig_len,
                       msgs, msg_off, msg_len, base, m, pre_status, status, ws, (flags & 1u) ? 0u : 1u);
    const uint64_t nt = (m + kEcInvBatch - 1) / kEcInvBatch;
    hipLaunchKernelGGL(ecdsa_inv_kernel, dim3((uint32_t)((nt + 255) / 256)), dim3(256), 0, s, base, m, counters, ws);
    hipLaunchKernelGGL(ecdsa_ladder_idx_kernel<2>, g, dim3(256), 0, s, perm, counters, scheme, base, m, gk1, ws,
                       status);
    hipLaunchKernelGGL(ecdsa_ladder_idx_kernel<3>, g, dim3(256), 0, s, perm, counters, scheme, base, m, gr1, ws,
                       status);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (verdict)
    hipLaunchKernelGGL(verdict_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, status, n, verdict);
  return hipGetLastError();
}
