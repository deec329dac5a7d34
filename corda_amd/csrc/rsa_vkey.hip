// RSA_SHA256 verification against registered public keys (K18): part of rsa.hip's
// translation unit, whose kT-lane group layout, mont_mul, cond_sub and
// rsa_pss_check_kernel it shares unchanged (none of K8's code changes; the
// generic kernels compile as before). The record, the schedule and its host
// reference are in rsa_vkey.hpp.
//
// rsa_modexp_keyed_kernel<W>: a group of kT = 8 lanes per signature, as
// rsa_modexp_kernel<W>. A row's key is the record of slot key_id & 63 of the
// device's table; it is live when the record's id is the lane's and its width
// class is W. The group loads its windows of n, K and `in`, n' and e -- no Newton
// step, no bit-length scan, no doubling loop, no R^2 -- and runs acc = in; per
// bit of e below the top bit acc = mont(acc, acc) and, the bit set, acc =
// mont(acc, in); last acc = mont(acc, K), K = R^e mod n. K waits in LDS (L words
// a lane, 8 / 12 / 16 KiB a block) until that last product, when it takes the
// registers of `in`: the chain carries n, acc and one operand, as K8's does. The
// bit position is wave-uniform (the wave's longest e sets the schedule; a step no
// group needs is skipped), and every product goes through one instance of the
// multiplication loop, as in K8.
// No group returns before a shuffle: a row past the end, decided by the prep, of
// an unknown key or of another class loads and stores nothing of the key and runs
// every cross-lane step on K8's stand-ins (n = R - 1, in = 0, e = 1, K = 1). A
// null table makes every row unknown without a read; the slot is 6 bits of the
// id, so no index leaves the table.
//
// rsa_pss_prep_keyed_kernel: one lane per signature, as rsa_pss_prep_kernel, with
// the modulus' bit length and the class from the record.

namespace {

// the record of the lane's key if it is live in class W, else null
CDEV const uint32_t* rsa_vkey_record(const uint32_t* __restrict__ tab, uint32_t id, uint32_t W) {
  if (!tab) return nullptr;
  const uint32_t* rec = tab + (size_t)vkey_slot(id) * rsa::kVkeyRecWords;
  return (rec[rsa::kVkeyRecIdWord] == id && rec[rsa::kVkeyRecWordsWord] == W) ? rec : nullptr;
}

// out[row] = in[row]^e mod n of the key key_id[row] names, rows of W little-endian
// words. A row whose key is not live in class W, or with in >= n, gives a zero row
// and bad[row] = 1; a row with a nonzero skip[row] is left alone. in may alias out.
// kIdx (K20, the keyed list of a routed launch): the grid covers the launch's rows and
// nrows is not used; the list's length is read from *count, a block wholly past it
// returns at once, as a block, and group j below it takes row perm[j] of the launch;
// key_id is then route[], indexed by row like the rest. A keyed wave holds keyed rows only.
// The two forms are instances of one kernel, not of a device function the kernels
// inline: as a function's, K's wait in LDS is optimised away and K is carried in
// registers through the chain (83 / 146 / 158 VGPRs for 72 / 106 / 142, 5 / 3 / 3 waves
// per SIMD for 7 / 4 / 3).
template <int W, bool kIdx>
__global__ void __launch_bounds__(kBlock) rsa_modexp_keyed_kernel(const uint32_t* __restrict__ tab,
                                                                   const uint32_t* __restrict__ key_id,
                                                                   const uint32_t* in, uint64_t nrows, uint32_t* out,
                                                                   uint8_t* __restrict__ bad,
                                                                   const uint8_t* __restrict__ skip,
                                                                   const unsigned int* __restrict__ perm,
                                                                   const unsigned int* __restrict__ count) {
  constexpr int L = W / kT;
  if (kIdx) {
    nrows = *count;
    if (!rsa_route_idx_block_live(blockIdx.x, nrows)) return;
  }
  static_assert(W % kT == 0 && L % 4 == 0, "width class");
  const int gl = threadIdx.x & (kT - 1);
  const int gbase = (threadIdx.x & 63) & ~(kT - 1);
  uint64_t row = (uint64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kT;
  bool ok;
  if (kIdx) {
    ok = row < nrows;
    row = ok ? perm[row] : 0;
  } else {
    ok = row < nrows && !(skip && skip[row]);
  }
  const uint64_t base = row * W + (uint64_t)gl * L;
  const uint32_t* rec = ok ? rsa_vkey_record(tab, key_id[row], W) : nullptr;
  // K waits in LDS for the last product, each lane's words in a column of its own
  // (no lane reads another's: no barrier), so the loop below carries no register for it
  __shared__ uint32_t kst[L][kBlock];
  uint32_t n[L], acc[L], other[L];
  uint32_t e = 1, np = 1;  // the stand-ins: n = R - 1 (n' = 1), in = 0, e = 1, K = 1
#pragma unroll
  for (int i = 0; i < L; i++) {
    n[i] = 0xffffffffu;
    other[i] = 0;
    acc[i] = (gl == 0 && i == 0) ? 1u : 0u;
  }
  if (rec) {
    const uint4* kv = reinterpret_cast<const uint4*>(rec + rsa::kVkeyRecKWord + gl * L);
#pragma unroll
    for (int i = 0; i < L / 4; i++) {
      const uint4 v = kv[i];
      acc[4 * i] = v.x, acc[4 * i + 1] = v.y, acc[4 * i + 2] = v.z, acc[4 * i + 3] = v.w;
    }
    const uint4* nv = reinterpret_cast<const uint4*>(rec + rsa::kVkeyRecNWord + gl * L);
#pragma unroll
    for (int i = 0; i < L / 4; i++) {
      const uint4 v = nv[i];
      n[4 * i] = v.x, n[4 * i + 1] = v.y, n[4 * i + 2] = v.z, n[4 * i + 3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < L; i++) other[i] = in[base + i];
    e = rec[rsa::kVkeyRecEWord];
    np = rec[rsa::kVkeyRecNpWord];
  }
  {
    // the contract: in < n
    int c = 0;
#pragma unroll
    for (int i = 0; i < L; i++) c = other[i] > n[i] ? 1 : other[i] < n[i] ? -1 : c;
    const uint32_t g = group_bits(__ballot(c > 0), gbase), l = group_bits(__ballot(c < 0), gbase);
    const bool good = rec && g < l;
    if (!good) {
      e = 1;
      np = 1;
#pragma unroll
      for (int i = 0; i < L; i++) {
        n[i] = 0xffffffffu;
        other[i] = 0;
      }
    }
    if (ok && gl == 0 && bad) bad[row] = good ? 0 : 1;
    if (ok && !good) {
#pragma unroll
      for (int i = 0; i < L; i++) out[base + i] = 0;
    }
    ok = good;
  }
#pragma unroll
  for (int i = 0; i < L; i++) kst[i][threadIdx.x] = acc[i];
  // the wave's longest exponent sets the schedule
  uint32_t emax = e;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) emax = max(emax, (uint32_t)__shfl_xor((int)emax, off));
  const int topbit = 31 - __clz((int)__builtin_amdgcn_readfirstlane(emax));
#pragma unroll
  for (int i = 0; i < L; i++) acc[i] = other[i];
  // steps: per bit below the wave's top bit a square and a multiply by `in`, taken by
  // the groups that have met their own top bit; then acc * K for every group
  const int last = 2 * topbit;
  bool started = (e >> topbit) & 1u;
  for (int it = 0; it <= last; it++) {
    bool square = false, take = true;
    if (it < last) {
      const bool b = (e >> (topbit - 1 - (it >> 1))) & 1u;
      square = !(it & 1);
      take = started && (square || b);
      if (!square) started = started || b;  // a group's first set bit: acc is the base already
      if (!__any(take)) continue;
    } else {
#pragma unroll
      for (int i = 0; i < L; i++) other[i] = kst[i][threadIdx.x];  // the base's registers: no step needs it any more
    }
    uint32_t bsel[L], r[L];
#pragma unroll
    for (int i = 0; i < L; i++) bsel[i] = square ? acc[i] : other[i];
    mont_mul<L>(r, acc, bsel, n, np, gl, gbase);
#pragma unroll
    for (int i = 0; i < L; i++) acc[i] = take ? r[i] : acc[i];
  }
  if (ok) {
#pragma unroll
    for (int i = 0; i < L; i++) out[base + i] = acc[i];
  }
}

// One lane per signature: UNKNOWN_KEY for a key that is not live in class W (no
// record field beyond the id and the class is used), then EMPTY under doVerify
// rules, then BAD_SIG for a signature longer than the modulus (also every length
// beyond the slot: nothing past it is read); the signature as W little-endian
// words (zero for decided rows) and the modulus' bit length.
__global__ void __launch_bounds__(256) rsa_pss_prep_keyed_kernel(const uint32_t* __restrict__ tab,
                                                                 const uint32_t* __restrict__ key_id,
                                                                 const uint8_t* __restrict__ sigs,
                                                                 const uint16_t* __restrict__ sig_len,
                                                                 const uint64_t* __restrict__ msg_off,
                                                                 uint32_t msg_len, uint32_t W, uint64_t n,
                                                                 uint32_t flags, uint32_t* __restrict__ words,
                                                                 uint32_t* __restrict__ bits_out,
                                                                 uint8_t* __restrict__ st) {
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const uint32_t* rec = rsa_vkey_record(tab, key_id[row], W);
  const uint32_t bits = rec ? rec[rsa::kVkeyRecBitsWord] : 0u, sl = sig_len[row];
  const uint64_t ml = msg_off ? msg_off[row + 1] - msg_off[row] : msg_len;
  const uint32_t k = (bits + 7) / 8;
  uint8_t s = kStatusOk;
  if (!rec) s = kVerifyUnknownKey;
  else if (!(flags & CORDAHIP_FLAG_IS_VALID) && (sl == 0 || ml == 0)) s = kStatusEmpty;
  else if (sl > k) s = kStatusBadSig;
  const uint8_t* sg = sigs + row * 4ull * W;
  uint32_t* w = words + row * W;
  for (uint32_t i = 0; i < W; i++) {
    uint32_t v = 0;
    if (s == kStatusOk) {
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t sig_byte = 4 * i + q;  // significance
        if (sig_byte < sl) v |= (uint32_t)sg[sl - 1 - sig_byte] << (8 * q);
      }
    }
    w[i] = v;
  }
  bits_out[row] = bits;
  st[row] = s;
}

template <int W>
hipError_t launch_modexp_keyed(const uint32_t* tab, const uint32_t* key_id, const uint32_t* in, uint64_t n,
                               uint32_t* out, uint8_t* bad, const uint8_t* skip, hipStream_t s) {
  const uint64_t blocks = (n + kGroupsPerBlock - 1) / kGroupsPerBlock;
  hipLaunchKernelGGL((rsa_modexp_keyed_kernel<W, false>), dim3((uint32_t)blocks), dim3(kBlock), 0, s, tab, key_id, in,
                     n, out, bad, skip, (const unsigned int*)nullptr, (const unsigned int*)nullptr);
  return hipGetLastError();
}

hipError_t modexp_keyed_any(uint32_t W, const uint32_t* tab, const uint32_t* key_id, const uint32_t* in, uint64_t n,
                            uint32_t* out, uint8_t* bad, const uint8_t* skip, hipStream_t s) {
  switch (W) {
    case 64: return launch_modexp_keyed<64>(tab, key_id, in, n, out, bad, skip, s);
    case 96: return launch_modexp_keyed<96>(tab, key_id, in, n, out, bad, skip, s);
    case 128: return launch_modexp_keyed<128>(tab, key_id, in, n, out, bad, skip, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace

size_t rsa_vkey_bytes() { return rsa::kVkeyTableBytes; }

hipError_t launch_rsa_public_op_keyed(const uint32_t* tab, const uint32_t* key_id, const uint32_t* in, uint32_t W,
                                      uint64_t n, uint32_t* out, hipStream_t s) {
  for (uint64_t lo = 0; lo < n; lo += kMaxLaunchRows) {
    const uint64_t m = std::min(kMaxLaunchRows, n - lo);
    hipError_t e = modexp_keyed_any(W, tab, key_id + lo, in + lo * W, m, out + lo * W, nullptr, nullptr, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_rsa_verify_keyed(const uint32_t* tab, const uint32_t* key_id, const uint8_t* sigs,
                                   const uint16_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off,
                                   uint32_t msg_len, uint32_t W, uint64_t n, uint8_t* status,
                                   unsigned long long* verdict, uint8_t* ws, uint64_t ws_rows, uint32_t flags,
                                   hipStream_t s) {
  if (W != 64 && W != 96 && W != 128) return hipErrorInvalidValue;
  ws_rows = std::min(ws_rows, kMaxLaunchRows) / 64 * 64;  // launches start on verdict words
  if (n && !ws_rows) return hipErrorInvalidValue;
  uint32_t* words = reinterpret_cast<uint32_t*>(ws);
  uint32_t* bits = words + ws_rows * W;
  uint8_t* st = reinterpret_cast<uint8_t*>(bits + ws_rows);
  uint8_t* bad = st + ws_rows;
  for (uint64_t lo = 0; lo < n; lo += ws_rows) {
    const uint64_t m = std::min(ws_rows, n - lo);
    const dim3 grid((uint32_t)((m + 255) / 256));
    hipLaunchKernelGGL(rsa_pss_prep_keyed_kernel, grid, dim3(256), 0, s, tab, key_id + lo, sigs + lo * 4 * W,
                       sig_len + lo, msg_off ? msg_off + lo : nullptr, msg_len, W, m, flags, words, bits, st);
    hipError_t e = modexp_keyed_any(W, tab, key_id + lo, words, m, words, bad, st, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rsa_pss_check_kernel, grid, dim3(256), 0, s, words, bits, st, bad,
                       msg_off ? msgs : msgs + lo * msg_len, msg_off ? msg_off + lo : nullptr, msg_len, W, m,
                       status + lo, verdict ? verdict + lo / 64 : nullptr, (const unsigned int*)nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
