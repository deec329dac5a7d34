// Routing of RSA rows to the keyed modular exponentiation for gfx950 -- kernel K20.
//
// Part of rsa.hip's translation unit (included inside namespace cordahip, after
// rsa_vkey.hip): rsa_pss_prep_kernel, rsa_pss_check_kernel and the two
// exponentiation bodies are used as they are.
//
// With cordahip_vkey_set_routing_rsa on and a live RSA verification key on the
// device, every launch of rsa_verify_enqueue (runtime.cpp) is split on the GPU
// between the prep and the check: rows whose class, exponent and modulus are a live
// record's go to K18's exponentiation (rsa_modexp_keyed_kernel<W, true>, 18 products
// for e = 65537), the others to K8's (rsa_modexp_kernel<W, true>, 29 to 31). Both write
// the row's m words and contract flag where the unrouted kernel would, so the check
// kernel needs no change. The rule, the pass and the scratch layout are
// rsa_route.hpp. The host never reads a count back.

namespace {

// One lane per row (rsa_route.hpp). hdr: the scratch's header (the two list counts,
// cleared by the launcher); totals: the device's cumulative keyed / generic row
// counters. 1 KiB of LDS for the candidates. count (K24, the mixed device calls; null:
// every one of the n rows): the launch's rows, known on the device only and clipped to n
// before anything is indexed; rows at or past it enter neither list and neither total.
__global__ void __launch_bounds__(kRsaRouteBlock) rsa_route_kernel(const uint32_t* __restrict__ mod,
                                                                  const uint32_t* __restrict__ exp,
                                                                  const uint8_t* __restrict__ st, uint32_t W,
                                                                  uint64_t n, const uint32_t* __restrict__ tab,
                                                                  unsigned int* __restrict__ hdr,
                                                                  uint32_t* __restrict__ route,
                                                                  unsigned int* __restrict__ keyed,
                                                                  unsigned int* __restrict__ generic,
                                                                  unsigned long long* __restrict__ totals,
                                                                  const unsigned int* __restrict__ count) {
  __shared__ uint32_t cand[kVkeySlots * kRsaRouteCandWords];
  __shared__ uint32_t ncand_s;
  if (threadIdx.x < 64) {  // wave 0: one lane per slot, the live records in slot order
    const uint32_t slot = threadIdx.x;
    const uint32_t* rec = tab + (size_t)slot * rsa::kVkeyRecWords;
    const bool live = slot < kVkeySlots && rsa_route_rec_live(rec);
    const unsigned long long b = __ballot(live);
    if (live) rsa_route_put(cand, route_rank(b, slot), rec);
    if (slot == 0) ncand_s = (uint32_t)__popcll(b);
  }
  __syncthreads();
  const uint32_t ncand = ncand_s;
  if (count) n = route_count_clip(*count, n);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i = rsa_route_row(blockIdx.x, threadIdx.x);
  bool is_keyed = false, is_generic = false, listed = false;
  if (i < n) {
    const uint32_t id = rsa_route_match(W, exp[i], mod + i * W, cand, ncand, tab);
    route[i] = id;
    is_keyed = id != kVkeyNoId;
    is_generic = !is_keyed;
    listed = st[i] == kStatusOk;
  }
  const unsigned long long mk = __ballot(is_keyed), mg = __ballot(is_generic);
  const unsigned long long lk = __ballot(is_keyed && listed), lg = __ballot(is_generic && listed);
  unsigned int sk = 0, sg = 0;
  if (lane == 0) {
    if (lk) sk = atomicAdd(&hdr[kRsaRouteCntKeyed], (unsigned int)__popcll(lk));
    if (lg) sg = atomicAdd(&hdr[kRsaRouteCntGeneric], (unsigned int)__popcll(lg));
    if (mk) atomicAdd(&totals[0], (unsigned long long)__popcll(mk));
    if (mg) atomicAdd(&totals[1], (unsigned long long)__popcll(mg));
  }
  sk = __shfl(sk, 0);
  sg = __shfl(sg, 0);
  if (is_keyed && listed) keyed[sk + route_rank(lk, lane)] = (unsigned int)i;
  if (is_generic && listed) generic[sg + route_rank(lg, lane)] = (unsigned int)i;
}

template <int W>
hipError_t launch_modexp_routed(const uint32_t* mod, const uint32_t* exp, uint32_t* words, uint64_t m, uint8_t* bad,
                                const uint32_t* tab, const unsigned int* hdr, const uint32_t* route,
                                const unsigned int* keyed, const unsigned int* generic, bool keyed_half,
                                hipStream_t s) {
  const dim3 grid((uint32_t)rsa_route_idx_blocks(m));
  if (keyed_half)
    hipLaunchKernelGGL((rsa_modexp_keyed_kernel<W, true>), grid, dim3(kBlock), 0, s, tab, route, words, (uint64_t)0,
                       words, bad, (const uint8_t*)nullptr, keyed, hdr + kRsaRouteCntKeyed);
  else
    hipLaunchKernelGGL((rsa_modexp_kernel<W, true>), grid, dim3(kBlock), 0, s, mod, exp, words, (uint64_t)0, words, bad,
                       (const uint8_t*)nullptr, generic, hdr + kRsaRouteCntGeneric);
  return hipGetLastError();
}

hipError_t modexp_routed_any(uint32_t W, const uint32_t* mod, const uint32_t* exp, uint32_t* words, uint64_t m,
                             uint8_t* bad, const uint32_t* tab, const unsigned int* hdr, const uint32_t* route,
                             const unsigned int* keyed, const unsigned int* generic, bool keyed_half, hipStream_t s) {
  switch (W) {
    case 64: return launch_modexp_routed<64>(mod, exp, words, m, bad, tab, hdr, route, keyed, generic, keyed_half, s);
    case 96: return launch_modexp_routed<96>(mod, exp, words, m, bad, tab, hdr, route, keyed, generic, keyed_half, s);
    case 128:
      return launch_modexp_routed<128>(mod, exp, words, m, bad, tab, hdr, route, keyed, generic, keyed_half, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

size_t rsa_route_scratch_bytes(uint64_t cap_rows) { return (size_t)rsa_route_scratch_words(cap_rows) * 4; }

// the rows a launch takes: what launch_rsa_pss_verify makes of the workspace's rows
uint64_t rsa_launch_rows(uint64_t ws_rows) { return std::min(ws_rows, kMaxLaunchRows) / 64 * 64; }

// One launch of a routed batch in three parts, so that the caller can hold the key
// table's lock around the middle one only (runtime.cpp rsa_verify_enqueue). m rows
// from row lo of the batch, m at most rsa_launch_rows(ws_rows); scratch: the
// workspace's, rsa_route_scratch_bytes(cap_rows), cap_rows >= m.
//   head:  the prep
//   keyed: the counts cleared, the route pass, K18's exponentiation over the keyed list
//   tail:  K8's exponentiation over the generic list, the check; routed false (no key was
//          live any more when the middle part's turn came): K8's over every row, as unrouted
// count (K24, K23's convention; null for the dense calls): the batch's rows are known on
// the device only, n is the host's bound. The head leaves the launch's rows, clipped to
// m, in *launch_count (rsa_launch_count_kernel); the prep, the route pass and the check
// stop there, and an unrouted tail runs K8's indexed instance over iota.
hipError_t launch_rsa_routed_head(const uint32_t* mod, const uint32_t* exp, const uint8_t* sigs,
                                  const uint16_t* sig_len, const uint64_t* msg_off, uint32_t msg_len, uint32_t W,
                                  uint64_t lo, uint64_t m, const uint8_t* pre, uint8_t* ws, uint64_t ws_rows,
                                  uint32_t flags, hipStream_t s, const unsigned int* count,
                                  unsigned int* launch_count) {
  if (W != 64 && W != 96 && W != 128) return hipErrorInvalidValue;
  ws_rows = rsa_launch_rows(ws_rows);
  if (!m || m > ws_rows || (count && !launch_count)) return hipErrorInvalidValue;
  uint32_t* words = reinterpret_cast<uint32_t*>(ws);
  uint32_t* bits = words + ws_rows * W;
  uint8_t* st = reinterpret_cast<uint8_t*>(bits + ws_rows);
  const dim3 grid((uint32_t)((m + 255) / 256));
  if (count) hipLaunchKernelGGL(rsa_launch_count_kernel, dim3(1), dim3(1), 0, s, count, lo, m, launch_count);
  hipLaunchKernelGGL(rsa_pss_prep_kernel, grid, dim3(256), 0, s, mod + lo * W, exp + lo, sigs + lo * 4 * W,
                     sig_len + lo, msg_off ? msg_off + lo : nullptr, msg_len, W, m, pre ? pre + lo : nullptr, flags,
                     words, bits, st, count ? (const unsigned int*)launch_count : nullptr);
  return hipGetLastError();
}

hipError_t launch_rsa_routed_keyed(const uint32_t* mod, const uint32_t* exp, uint32_t W, uint64_t lo, uint64_t m,
                                   const uint32_t* tab, uint8_t* ws, uint64_t ws_rows, uint32_t* scratch,
                                   uint64_t cap_rows, unsigned long long* totals, hipStream_t s,
                                   const unsigned int* launch_count) {
  ws_rows = rsa_launch_rows(ws_rows);
  if (!m || m > ws_rows || m > cap_rows || !tab || !scratch || !totals) return hipErrorInvalidValue;
  uint32_t* words = reinterpret_cast<uint32_t*>(ws);
  uint8_t* st = reinterpret_cast<uint8_t*>(words + ws_rows * W + ws_rows);
  uint8_t* bad = st + ws_rows;
  hipError_t e = hipMemsetAsync(scratch, 0, 2 * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  uint32_t* route = scratch + rsa_route_off_route(cap_rows);
  unsigned int* keyed = scratch + rsa_route_off_keyed(cap_rows);
  unsigned int* generic = scratch + rsa_route_off_generic(cap_rows);
  hipLaunchKernelGGL(rsa_route_kernel, dim3((uint32_t)((m + kRsaRouteBlock - 1) / kRsaRouteBlock)),
                     dim3(kRsaRouteBlock), 0, s, mod + lo * W, exp + lo, st, W, m, tab, scratch, route, keyed, generic,
                     totals, launch_count);
  e = hipGetLastError();
  return e ? e
           : modexp_routed_any(W, mod + lo * W, exp + lo, words, m, bad, tab, scratch, route, keyed, generic, true, s);
}

hipError_t launch_rsa_routed_tail(const uint32_t* mod, const uint32_t* exp, const uint8_t* msgs,
                                  const uint64_t* msg_off, uint32_t msg_len, uint32_t W, uint64_t lo, uint64_t m,
                                  uint8_t* status, unsigned long long* verdict, uint8_t* ws, uint64_t ws_rows,
                                  const uint32_t* scratch, uint64_t cap_rows, bool routed, hipStream_t s,
                                  const unsigned int* launch_count, const unsigned int* iota) {
  ws_rows = rsa_launch_rows(ws_rows);
  if (!m || m > ws_rows || (routed && (m > cap_rows || !scratch))) return hipErrorInvalidValue;
  if (launch_count && !routed && !iota) return hipErrorInvalidValue;
  uint32_t* words = reinterpret_cast<uint32_t*>(ws);
  uint32_t* bits = words + ws_rows * W;
  uint8_t* st = reinterpret_cast<uint8_t*>(bits + ws_rows);
  uint8_t* bad = st + ws_rows;
  hipError_t e =
      routed ? modexp_routed_any(W, mod + lo * W, exp + lo, words, m, bad, nullptr, scratch,
                                 scratch + rsa_route_off_route(cap_rows), scratch + rsa_route_off_keyed(cap_rows),
                                 scratch + rsa_route_off_generic(cap_rows), false, s)
      : launch_count ? modexp_counted_any(W, mod + lo * W, exp + lo, words, m, bad, iota, launch_count, s)
                     : modexp_any(W, mod + lo * W, exp + lo, words, m, words, bad, st, s);
  if (e != hipSuccess) return e;
  const dim3 grid((uint32_t)((m + 255) / 256));
  hipLaunchKernelGGL(rsa_pss_check_kernel, grid, dim3(256), 0, s, words, bits, st, bad,
                     msg_off ? msgs : msgs + lo * msg_len, msg_off ? msg_off + lo : nullptr, msg_len, W, m, status + lo,
                     verdict ? verdict + lo / 64 : nullptr, launch_count);
  return hipGetLastError();
}
