// Routing of Ed25519 lanes to the keyed verifier for gfx950 -- kernel K14.
//
// With cordahip_vkey_set_routing on and a live Ed25519 verification key on the
// device, every batch that reaches ed_verify_enqueue (runtime.cpp) is split on the
// GPU: lanes whose 32 key bytes equal a live record's Abyte go to K12
// (ed25519_vkey.hip, indexed instance), the others to K1 (ed25519.hip /
// ed25519_ladder.hip, indexed instances). This file holds the partition pass and the
// verdict pass that follows the two engines; the match rule and the scratch layout
// are ed25519_route.hpp. The host never reads a count back: the indexed kernels take
// their lane counts from the scratch header.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ed25519_route.hpp"
#include "status.hpp"

namespace cordahip {

// scratch: ed25519_route.hpp's layout for n lanes, its two counts zeroed by the
// launcher. totals: the device's cumulative keyed / generic lane counters.
// count (K24, the mixed device calls; null: every one of the n lanes): the rows to
// partition are known on the device only. It is clipped to n, the bound the launch and
// the scratch were sized for, before anything is indexed; rows at or past it enter
// neither list and neither total.
__global__ void __launch_bounds__(256) ed25519_route_kernel(const uint8_t* __restrict__ keys, uint64_t n,
                                                           const uint32_t* __restrict__ vtab,
                                                           uint32_t* __restrict__ scratch,
                                                           unsigned long long* __restrict__ totals,
                                                           const uint32_t* __restrict__ count) {
  __shared__ uint32_t recs[kVkeySlots * kRouteRecWords];
  __shared__ uint32_t nlive_s;
  const uint32_t lane = threadIdx.x & 63;
  if (threadIdx.x < kVkeySlots) {  // wave 0: one record per lane, gathered in slot order
    const uint32_t* rec = vtab + kVkeyRecBase + threadIdx.x * kVkeyRecWords;
    const bool live = route_rec_live(rec);
    const unsigned long long b = __ballot(live);
    if (live) {
      uint32_t* o = recs + route_rank(b, lane) * kRouteRecWords;
#pragma unroll
      for (int q = 0; q < 8; q++) o[q] = rec[kVkeyRecAbyte + q];
      o[8] = rec[kVkeyRecId];
    }
    if (threadIdx.x == 0) nlive_s = (uint32_t)__popcll(b);
  }
  __syncthreads();
  const uint32_t nlive = nlive_s;
  const uint64_t m = count ? route_count_clip(*count, n) : n;
  uint32_t* route = scratch + route_off_route(n);
  uint32_t* keyed = scratch + route_off_keyed(n);
  uint32_t* generic = scratch + route_off_generic(n);
  uint32_t id[kRouteIter];
  uint32_t nk = 0, ng = 0;
#pragma unroll
  for (int it = 0; it < kRouteIter; it++) {
    const uint64_t i = route_tile_lane(blockIdx.x, it, threadIdx.x);
    id[it] = kVkeyNoId;
    if (i < m) {
      const uint4* k4 = reinterpret_cast<const uint4*>(keys + i * 32);
      const uint4 a = k4[0], b = k4[1];
      const uint32_t key[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      id[it] = route_match(key, recs, nlive);
      route[i] = id[it];
    }
    nk += (uint32_t)__popcll(__ballot(i < m && id[it] != kVkeyNoId));
    ng += (uint32_t)__popcll(__ballot(i < m && id[it] == kVkeyNoId));
  }
  // the wave's range of each list: one atomic per list (and per cumulative counter)
  uint32_t sk = 0, sg = 0;
  if (lane == 0) {
    if (nk) {
      sk = atomicAdd(&scratch[kRouteCntKeyed], nk);
      atomicAdd(&totals[0], (unsigned long long)nk);
    }
    if (ng) {
      sg = atomicAdd(&scratch[kRouteCntGeneric], ng);
      atomicAdd(&totals[1], (unsigned long long)ng);
    }
  }
  sk = __shfl(sk, 0);
  sg = __shfl(sg, 0);
#pragma unroll
  for (int it = 0; it < kRouteIter; it++) {
    const uint64_t i = route_tile_lane(blockIdx.x, it, threadIdx.x);
    const bool in = i < m, hit = in && id[it] != kVkeyNoId, miss = in && id[it] == kVkeyNoId;
    const unsigned long long bk = __ballot(hit), bg = __ballot(miss);
    if (hit) keyed[sk + route_rank(bk, lane)] = (uint32_t)i;
    if (miss) generic[sg + route_rank(bg, lane)] = (uint32_t)i;
    sk += (uint32_t)__popcll(bk);
    sg += (uint32_t)__popcll(bg);
  }
}

// The verdict words of a routed batch: a permuted wave owns no word, so they are
// gathered from the final statuses (bit = status OK, bits past n zero).
__global__ void __launch_bounds__(256) ed25519_status_verdict_kernel(const uint8_t* __restrict__ status, uint64_t n,
                                                                    unsigned long long* __restrict__ verdict) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long m = __ballot(i < n && status[i] == kStatusOk);
  if ((threadIdx.x & 63) == 0 && i < n) verdict[i >> 6] = m;
}

// what the runtime allocates for a batch of n lanes (a capacity: ed25519_route.hpp)
size_t ed25519_route_scratch_bytes(uint64_t n) {
  return (size_t)route_scratch_words(route_scratch_cap_lanes(n)) * sizeof(uint32_t);
}
uint64_t ed25519_route_max_lanes() { return kRouteMaxLanes; }

hipError_t launch_ed25519_route(const uint8_t* keys, uint64_t n, const uint32_t* vtab, uint32_t* scratch,
                                unsigned long long* totals, hipStream_t s, const uint32_t* count) {
  if (n == 0 || n > kRouteMaxLanes || !vtab || !scratch || !totals) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(scratch, 0, 2 * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const uint64_t blocks = (n + kRouteTile - 1) / kRouteTile;
  hipLaunchKernelGGL(ed25519_route_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, keys, n, vtab, scratch, totals,
                     count);
  return hipGetLastError();
}

hipError_t launch_ed25519_status_verdict(const uint8_t* status, uint64_t n, unsigned long long* verdict,
                                         hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ed25519_status_verdict_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, status, n, verdict);
  return hipGetLastError();
}

}  // namespace cordahip
