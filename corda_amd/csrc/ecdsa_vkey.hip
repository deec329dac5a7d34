// ECDSA (ECDSA_SECP256K1_SHA256 = 2, ECDSA_SECP256R1_SHA256 = 3) batch
// verification against registered public keys for gfx950 -- kernel K13.
//
// Part of ecdsa.hip's translation unit (included at its end, inside namespace
// cordahip): the field, point, key-decode, DER and x_check functions of the
// generic verifier K2 are used as they are, and the generic kernels are not
// touched.
//
// Replaces, per lane, Crypto.doVerify / isValid for the two ECDSA schemes
// (Crypto.kt:472-541 -> BouncyCastle ECDSASigner.verifySignature) for a handful
// of long-lived keys (HSM-held notary and oracle keys, doorman and node-CA
// certificate issuers) and many signatures. A key is registered once
// (ecdsa_vkey_build_kernel: BC's SEC1 decode, then the window table [d 256^j]Q,
// d = 1..128, j = 0..31, ecdsa_vkey.hpp); a lane then computes
//   P = [u1]G + [u2]Q,  u1 = e / s, u2 = r / s,  and decides x(P) mod n == r
// as 64 mixed additions over signed 8-bit digits of u1 (the curve's base-point
// table) and u2 (the key's table): no doubling, no key decode, no per-lane
// table, no per-lane workspace, no field inversion (x_check compares
// projectively); s^-1 mod n is a per-lane Fermat inversion.
//
// Nothing here is secret: the gathers are indexed by the lane's own digits.
// Oracle: oracle/bc_ecdsa.py, oracle/c/ecdsa.c. Geometry: ecdsa_vkey.hpp (included
// by ecdsa.hip, outside the namespace).

// ---------------------------------------------------------------------------
// Registration, once per key and device: thread g builds the entry
// [d 256^j]Q, j = g / 128, d = g % 128 + 1 -- 8 j doublings of Q, a
// double-and-add by d, one inversion, canonical coordinates -- so the 4,096
// normalisations run in 4,096 lanes. d 256^j <= 2^255 < n and n is prime, so no
// entry is the point at infinity. The SEC1 bytes are in the table's scratch
// words; word kEcVkeyOkWord answers whether they decode (decode_key: BC's
// ECCurve.decodePoint). A key that does not decode writes neither a table nor a
// record. slot >= kVkeySlots: the table [d 256^j]G of the curve's base point
// instead (once per device and curve, with its first key): no key bytes, no record.
template <class C, int S>
__global__ void __launch_bounds__(64) ecdsa_vkey_build_kernel(uint32_t* __restrict__ vtab, uint32_t slot,
                                                              uint32_t key_id, uint32_t key_len) {
  using F = typename C::F;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= kVkeyDigits * kVkeyEntries) return;
  const int j = g / kVkeyEntries, d = g % kVkeyEntries + 1;
  jpt Q;
  if (slot >= kVkeySlots) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
      Q.X.v[i] = F::gxm(i);
      Q.Y.v[i] = F::gym(i);
    }
    f29_const_one<F>(Q.Z);
    Q.inf = false;
  } else {
    const bool ok = key_len <= kEcVkeyMaxKeyBytes &&
                    decode_key<C>(Q, reinterpret_cast<const uint8_t*>(vtab + kEcVkeyKeyWord), key_len);
    if (g == 0) {
      vtab[kEcVkeyOkWord] = ok ? 1u : 0u;
      if (ok) {
        uint32_t* rec = vtab + kEcVkeyRecBase + slot * kEcVkeyRecWords;
        rec[kEcVkeyRecScheme] = (uint32_t)S;
        rec[kEcVkeyRecId] = key_id;
        rec[kEcVkeyRecLive] = 1u;
      }
    }
    if (!ok) return;
  }
#pragma unroll 1
  for (int t = 0; t < 8 * j; t++) jdbl<C>(Q, Q);
  jpt R;
  R.inf = true;
#pragma unroll 1
  for (int bit = 7; bit >= 0; bit--) {
    jdbl<C>(R, R);
    if ((d >> bit) & 1) jadd<C>(R, R, Q);
  }
  f29 zi, zi2, x, y;
  f29_pow_const<F, typename C::Pm2>(zi, R.Z);
  f29_sqr<F>(zi2, zi);
  f29_mul<F>(x, R.X, zi2);
  f29_mul<F>(zi2, zi2, zi);
  f29_mul<F>(y, R.Y, zi2);
  f29_canon<F>(x, x);
  f29_canon<F>(y, y);
  uint32_t w[kEcVkeyEntryWords];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    w[i] = x.v[i];
    w[9 + i] = y.v[i];
  }
  w[18] = w[19] = 0;
  uint4* o4 = reinterpret_cast<uint4*>(vtab + (size_t)slot * kEcVkeyTableWords + ec_vkey_entry_word(j, d));
#pragma unroll
  for (int q = 0; q < 5; q++) o4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

// ---------------------------------------------------------------------------
// The lane's two biased scalars and r live in LDS, word-major, one column per
// thread (word w at col[w * 256]): a round reads one word of each, and the 24
// VGPRs they would pin across the loop go to the additions. Only the thread's
// own column is ever read, so no barrier is needed.
// ec_vkey_fetch: the entry, in table tab, of digit j of the biased scalar t
// (issued one addition ahead of its use); returns the digit. A zero digit reads
// the entry of d = 1 and its addition is skipped.
CDEV int ec_vkey_fetch(f29& x, f29& y, const uint32_t* __restrict__ tab, const uint32_t* t, int j) {
  const int d = vkey_digit(t[(j >> 2) * 256], j);
  const int ad = d < 0 ? -d : d;
  const uint4* e = reinterpret_cast<const uint4*>(tab + ec_vkey_entry_word(j, ad ? ad : 1));
  uint32_t w[20];
#pragma unroll
  for (int q = 0; q < 5; q++) {
    const uint4 v = e[q];
    w[4 * q] = v.x;
    w[4 * q + 1] = v.y;
    w[4 * q + 2] = v.z;
    w[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int i = 0; i < 9; i++) {
    x.v[i] = w[i];
    y.v[i] = w[9 + i];
  }
  return d;
}

// K13, one instance per curve; a call launches the instance of every curve that
// has a live key on the device (the P-256 one when none has: it then only writes
// UNKNOWN_KEY). Messages: moff / mlen non-null: lane i's message is mlen[i]
// bytes at msgs + moff[i]; else dense rows of msg_len bytes. Signatures: DER in
// 72-byte slots with their lengths. Statuses by precedence: UNKNOWN_KEY (the
// record of the id's slot holds another id, or none; such a lane reads nothing
// but that record), pre[i] when non-zero (the host form's decision on a
// signature longer than its slot), EMPTY (doVerify rules), MALFORMED_SIG (DER),
// BAD_SIG, OK. A lane whose key is of the other curve is left to that curve's
// instance. jmadd keeps its exceptional branches (accumulator equal to the
// entry, its inverse, at infinity): a sum without doublings reaches them.
//
// The body serves two kernels. kIdx false: K13 itself, lane i is thread i. kIdx true:
// the routed instance (K15, ecdsa_route.hpp): thread j below n takes lane
// i = list[j], key_id is the route array (indexed by lane), and moff is the generic
// engine's CSR offsets (the message's length is moff[i + 1] - moff[i]; mlen unused).
template <int S, bool kIdx>
CDEV void ec_verify_keyed_lane(const uint32_t* __restrict__ key_id, const unsigned int* __restrict__ list,
                               const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ sig_len,
                               const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ moff,
                               const uint32_t* __restrict__ mlen, uint32_t msg_len, uint64_t n,
                               const uint8_t* __restrict__ pre, uint32_t empty_is_error,
                               const uint32_t* __restrict__ vtab, uint8_t* __restrict__ status) {
  using C = Curve<S>;
  using N = typename C::N;
  using F = typename C::F;
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t i = kIdx ? list[j] : j;
  __shared__ uint32_t sk[24][256];  // u1 and u2, biased, and r: only the thread's own column is read
  const uint32_t id = key_id[i];
  const uint32_t slot = vkey_slot(id);
  if (!vtab || id == kVkeyNoId) {
    status[i] = kVerifyUnknownKey;
    return;
  }
  {
    const uint32_t* rec = vtab + kEcVkeyRecBase + slot * kEcVkeyRecWords;
    if (rec[kEcVkeyRecId] != id || rec[kEcVkeyRecLive] != 1u) {
      status[i] = kVerifyUnknownKey;
      return;
    }
    if (rec[kEcVkeyRecScheme] != (uint32_t)S) return;  // the other curve's instance decides
  }
  const uint64_t ml = moff ? (kIdx ? moff[i + 1] - moff[i] : (uint64_t)mlen[i]) : msg_len;
  const uint8_t* msg = moff ? msgs + moff[i] : msgs + i * (uint64_t)msg_len;
  const uint8_t* sig = sigs + i * 72;
  uint32_t sl = sig_len[i];
  uint8_t st = pre ? pre[i] : kStatusOk;
  // a DER signature longer than its 72-byte slot: ecdsa_prep_kernel's rule
  if (sl > 72 && st == kStatusOk) st = (ml == 0 && empty_is_error) ? kStatusEmpty : kStatusMalformedSig;
  if (sl > 72) sl = 72;
  bool neg1 = false, neg2 = false;
  if (st == kStatusOk) {
    st = kEcPending;
    u256 r, s;
    if (empty_is_error && (sl == 0 || ml == 0)) {
      st = kStatusEmpty;  // doVerify: Crypto.kt:475-476 (isValid: DER decode / hash as usual)
    } else {
      DerInt dr, ds;
      if (!der_decode_sig(sig, sl, dr, ds)) {
        st = kStatusMalformedSig;
      } else {
#pragma unroll
        for (int q = 0; q < 8; q++) {
          r.v[q] = dr.v[q];
          s.v[q] = ds.v[q];
        }
        const u256 nm = mod_m<N>();
        if (dr.neg || dr.big || ds.neg || ds.big || u256_iszero(r) || u256_iszero(s) || u256_geq(r, nm) ||
            u256_geq(s, nm))
          st = kStatusBadSig;
      }
    }
    if (st == kEcPending) {
      uint32_t hw[8];
      sha256_bytes(hw, msg, ml);
      u256 e, t, w, u1, u2;
#pragma unroll
      for (int q = 0; q < 8; q++) e.v[q] = hw[7 - q];
      if (!u256_sub(t, e, mod_m<N>())) e = t;
      to_mont<N>(t, s);
      mont_pow_const<N, typename C::Nm2>(w, t);  // s^-1, Montgomery form
      mont_mul<N>(u1, e, w);                     // plain e / s (one Montgomery factor cancels)
      mont_mul<N>(u2, r, w);
      // the header's own sign split and bias: what tools/ec_vkey_check.cpp checks on the host
      const u256 nm = mod_m<N>();
      uint32_t m1[8], m2[8], b1[8], b2[8];
      neg1 = ec_vkey_split_sign(m1, u1.v, nm.v);
      neg2 = ec_vkey_split_sign(m2, u2.v, nm.v);
      ec_vkey_bias(b1, m1);
      ec_vkey_bias(b2, m2);
#pragma unroll
      for (int q = 0; q < 8; q++) {
        sk[q][threadIdx.x] = b1[q];
        sk[8 + q][threadIdx.x] = b2[q];
        sk[16 + q][threadIdx.x] = r.v[q];
      }
    }
  }
  if (st == kEcPending) {
    const uint32_t* t1 = &sk[0][threadIdx.x];
    const uint32_t* t2 = &sk[8][threadIdx.x];
    const uint32_t* gtab = vtab + (size_t)ec_vkey_base_slot(S) * kEcVkeyTableWords;
    const uint32_t* qtab = vtab + (size_t)slot * kEcVkeyTableWords;
    // P = sum of up to 64 table entries (order: ecdsa_vkey.hpp), two per round:
    // the base point's digit j, the key's digit j. Each gather is issued one
    // addition ahead of its use.
    jpt acc;
    acc.inf = true;
    f29 cx, cy, nx, ny;
    int dc = ec_vkey_fetch(cx, cy, gtab, t1, kVkeyDigits - 1);
#pragma unroll 1
    for (int j = kVkeyDigits - 1; j >= 0; j--) {
      const int dn = ec_vkey_fetch(nx, ny, qtab, t2, j);
      if (dc) {
        f29_cneg_loose<F>(cy, (dc < 0) != neg1);
        jmadd<C>(acc, acc, cx, cy);
      }
      // the last round gathers digit 0 again and drops it
      dc = ec_vkey_fetch(cx, cy, gtab, t1, j > 0 ? j - 1 : 0);
      if (dn) {
        f29_cneg_loose<F>(ny, (dn < 0) != neg2);
        jmadd<C>(acc, acc, nx, ny);
      }
    }
    u256 r;
#pragma unroll
    for (int q = 0; q < 8; q++) r.v[q] = sk[16 + q][threadIdx.x];
    st = x_check<C>(acc, r);
  }
  status[i] = st;
}

template <int S>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) ecdsa_verify_keyed_kernel(
    const uint32_t* __restrict__ key_id, const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ sig_len,
    const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ moff, const uint32_t* __restrict__ mlen,
    uint32_t msg_len, uint64_t n, const uint8_t* __restrict__ pre, uint32_t empty_is_error,
    const uint32_t* __restrict__ vtab, uint8_t* __restrict__ status) {
  ec_verify_keyed_lane<S, false>(key_id, nullptr, sigs, sig_len, msgs, moff, mlen, msg_len, n, pre, empty_is_error,
                                 vtab, status);
}

// ---------------------------------------------------------------------------
// host-side launchers (called by cordahip.cpp)
size_t ecdsa_vkey_bytes() { return (size_t)kEcVkeyAllWords * sizeof(uint32_t); }

// scheme 2 / 3; slot < kVkeySlots: the key whose SEC1 bytes are in the scratch words,
// else the curve's base-point table
hipError_t launch_ecdsa_vkey_build(uint32_t* vtab, uint32_t scheme, uint32_t slot, uint32_t key_id, uint32_t key_len,
                                   hipStream_t s) {
  const dim3 g(kVkeyDigits * kVkeyEntries / 64);
  if (scheme == 2)
    hipLaunchKernelGGL((ecdsa_vkey_build_kernel<Curve<2>, 2>), g, dim3(64), 0, s, vtab, slot, key_id, key_len);
  else
    hipLaunchKernelGGL((ecdsa_vkey_build_kernel<Curve<3>, 3>), g, dim3(64), 0, s, vtab, slot, key_id, key_len);
  return hipGetLastError();
}

// live_k1 / live_r1: whether the device holds a live key of that curve
hipError_t launch_ecdsa_verify_keyed(const uint32_t* key_id, const uint8_t* sigs, const uint8_t* sig_len,
                                     const uint8_t* msgs, const uint64_t* moff, const uint32_t* mlen, uint32_t msg_len,
                                     uint64_t n, const uint8_t* pre, uint32_t flags, const uint32_t* vtab,
                                     bool live_k1, bool live_r1, uint8_t* status, unsigned long long* verdict,
                                     hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)blocks);
  const uint32_t eie = (flags & 1u) ? 0u : 1u;
  if (live_k1)
    hipLaunchKernelGGL(ecdsa_verify_keyed_kernel<2>, grid, dim3(256), 0, s, key_id, sigs, sig_len, msgs, moff, mlen,
                       msg_len, n, pre, eie, vtab, status);
  if (live_r1 || !live_k1)
    hipLaunchKernelGGL(ecdsa_verify_keyed_kernel<3>, grid, dim3(256), 0, s, key_id, sigs, sig_len, msgs, moff, mlen,
                       msg_len, n, pre, eie, vtab, status);
  if (verdict) hipLaunchKernelGGL(verdict_kernel, grid, dim3(256), 0, s, status, n, verdict);
  return hipGetLastError();
}
