// ECDSA (ECDSA_SECP256K1_SHA256 = 2, ECDSA_SECP256R1_SHA256 = 3) batch signing with
// registered keys for gfx950 -- kernel K17.
//
// Part of ecdsa.hip's translation unit (included at its end, inside namespace
// cordahip): the field and point arithmetic, the ring mod n, der_put_int and SHA-256
// of the verifier are used as they are, and the generic kernels are not touched.
//
// Replaces, per lane, Crypto.doSign for the two ECDSA schemes (Crypto.kt:394-401 ->
// JCA "SHA256withECDSA" -> BouncyCastle ECDSASigner.generateSignature) with the
// deterministic nonce of RFC 6979 (BouncyCastle's HMacDSAKCalculator) for a handful
// of long-lived keys and many messages:
//   h1 = SHA-256(m), e = int(h1) mod n, k = the RFC 6979 nonce of (d, h1),
//   r = x([k]G) mod n, s = k^-1 (e + d r) mod n, DER SEQUENCE { r, s }; s is not
//   normalised to the low half (BC 1.57 does not; every verifier takes both halves).
// An ECDSA signature is judged by its verifier, not by its bytes: BC's default signer
// draws a random nonce, so no implementation can match its bytes, and every verifier
// accepts these. The scalar side -- nonce, k' = min(k, n - k), digits -- is
// ecdsa_sign_core.hpp, which tools/ecdsa_sign_check.cpp runs on the host.
//
// Secrets are d, k, k', the digits, k^-1 and the HMAC states. No address and no branch
// depends on them:
//   [k']G is 64 mixed additions from the comb table [d 16^j]G, d = 1..8, j = 0..63:
//     no doublings. For position j every lane reads all 8 entries of that position
//     (the addresses depend on the loop counter alone), keeps its own by a mask of
//     |d_j| == e and applies the sign by mask (ec_sign_select, ct_mask).
//   The addition never branches (jmadd_ct below).
//   k'^-1 mod n and Z^-1 mod p are the fixed chains mont_pow_const / f29_pow_const,
//     whose exponent is a compile-time constant; k'^-1 is negated by mask when k was
//     flipped. The reductions mod n end in selects (ecs_reduce_once, cond_sub_m).
//   The HMAC blocks have fixed lengths (ecdsa_sign_core.hpp).
// What does branch is public: the gate byte, the key id against the record, the
// message length (also in SHA-256's block loop over m), the DER lengths of r and s
// (they are the output), and the discard of a rejected candidate.

// ---------------------------------------------------------------------------
// comb table: thread g builds the entry [d 16^j]G, j = g / 8, d = g % 8 + 1
// (nothing here is secret: the branching jdbl / jadd serve)
template <class C>
__global__ void __launch_bounds__(64) ecdsa_sign_comb_kernel(uint32_t* __restrict__ tab) {
  using F = typename C::F;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= kCombDigits * kCombEntries) return;
  const int j = g / kCombEntries, d = g % kCombEntries + 1;
  jpt Q;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    Q.X.v[i] = F::gxm(i);
    Q.Y.v[i] = F::gym(i);
  }
  f29_const_one<F>(Q.Z);
  Q.inf = false;
#pragma unroll 1
  for (int t = 0; t < 4 * j; t++) jdbl<C>(Q, Q);
  jpt R;
  R.inf = true;
#pragma unroll 1
  for (int bit = 3; bit >= 0; bit--) {
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
  uint32_t w[kEcSignEntryWords];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    w[i] = x.v[i];
    w[9 + i] = y.v[i];
  }
  w[18] = w[19] = 0;
  uint4* o4 = reinterpret_cast<uint4*>(tab + ec_sign_entry_word(j, d));
#pragma unroll
  for (int q = 0; q < 5; q++) o4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}

// All ones when c holds, else zero, behind an empty asm: the optimizer sees an opaque
// word, so a selection written with it stays AND / OR arithmetic and cannot be turned
// back into control flow on the (secret) condition.
CDEV uint32_t ct_mask(bool c) {
  uint32_t m = 0u - (uint32_t)c;
  asm volatile("" : "+v"(m));
  return m;
}
CDEV uint32_t ct_sel(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }  // m ? a : b

// The entry of position j for the digit d in [-7, 8]: every entry of the position is
// read, the lane's own kept by mask; y is negated by mask (f29_cneg_loose's 4p - y, the
// operand form jmadd takes). d == 0 keeps the entry of 1, which jmadd_ct drops.
template <class F>
CDEV void ec_sign_select(f29& x, f29& y, const uint32_t* __restrict__ comb, int j, int d) {
  const int sgn = d >> 31;  // 0 or -1
  const uint32_t ad = (uint32_t)((d ^ sgn) - sgn);
  load_g(x, y, comb, comb_index(j, 1));
#pragma unroll
  for (int e = 2; e <= kCombEntries; e++) {
    f29 tx, ty;
    load_g(tx, ty, comb, comb_index(j, e));
    const uint32_t hit = ct_mask(ad == (uint32_t)e);
#pragma unroll
    for (int i = 0; i < 9; i++) {
      x.v[i] = ct_sel(hit, tx.v[i], x.v[i]);
      y.v[i] = ct_sel(hit, ty.v[i], y.v[i]);
    }
  }
  const uint32_t ng = ct_mask(sgn != 0);  // f29_cneg_loose's 4p - y, by mask
#pragma unroll
  for (int i = 0; i < 9; i++) y.v[i] = ct_sel(ng, F::sub4p(i) - y.v[i], y.v[i]);
}

// acc += (x2, y2) without a branch (madd-2007-bl as jmadd computes it): the general
// sum is computed whatever the operands are, and the result is selected among
//   the accumulator          (the digit is zero),
//   the entry lifted to Z = 1 (the accumulator is the point at infinity),
//   the sum                  (neither),
// by the two flags; acc_inf is updated the same way. A lane at infinity carries
// (1, 1, 1) in the accumulator, so every product sees operands within fp29.hpp's
// bounds and the discarded sum is merely meaningless.
// The cases the general formula does not cover -- the accumulator equal to the entry
// (a doubling) or to its inverse -- cannot occur. The comb runs from the top digit
// down; at position j the accumulator is [S]G with S = sum_{i > j} d_i 16^i, a
// multiple of 16^(j+1): S = 0 (infinity, handled by the flag), or
// |S| >= 16^(j+1) > 8 16^j >= |d_j 16^j|, so S != +-d_j 16^j as integers. And
// |S| <= k' + 16^(j+1) (the digits below position j + 1 sum to less than 16^(j+1) in
// absolute value), so |S +- d_j 16^j| < 2^255 + 1.5 * 2^252 < n: the non-zero integer
// S -+ d_j 16^j is not a multiple of n, i.e. [S]G != +-[d_j 16^j]G.
// tests/ecdsa_sign_model.py comb_mult runs the same selection with a chord-only
// addition that raises on either case.
// acc_inf and digit_zero are ct_mask words (all ones / zero).
template <class C>
CDEV void jmadd_ct(jpt& acc, uint32_t& acc_inf, const f29& x2, const f29& y2, uint32_t digit_zero) {
  using F = typename C::F;
  f29 z1z1, u2, h, hh, i, j, rr, v, t, x3, y3, z3;
  f29_sqr_mul_pair<F>(z1z1, acc.Z, t, y2, acc.Z);
  f29_mul_pair_s1s1<F>(h, x2, z1z1, acc.X, rr, t, z1z1, acc.Y);  // H = U2 - X1, R = S2 - Y1
  f29_add(rr, rr, rr);
  f29_add(t, acc.Z, acc.Z);
  f29_sqr_mul_pair<F>(hh, h, z3, t, h);  // HH, Z3 = 2 Z1 H
  f29_add(i, hh, hh);
  f29_add(i, i, i);  // I = 4 HH, < 8p
  f29_mul_pair<F>(j, h, i, v, acc.X, i);
  f29_sqr1_s3<F>(x3, rr, j, v, v);  // X3 = r^2 - J - 2 V
  f29_sub<F>(u2, v, x3);
  f29_neg2_norm<F>(t, j);
  f29_mul2<F>(y3, rr, u2, acc.Y, t);  // Y3 = r (V - X3) + Y1 (4p - 2J)
  f29 ly, one;
  f29_red<F>(ly, y2);  // y2 may be 4p - y: back to norm
  f29_const_one<F>(one);
  const uint32_t nz = ~digit_zero, lift = acc_inf & nz, sum = ~acc_inf & nz, keep = digit_zero;
#pragma unroll
  for (int q = 0; q < 9; q++) {
    acc.X.v[q] = (x3.v[q] & sum) | (x2.v[q] & lift) | (acc.X.v[q] & keep);
    acc.Y.v[q] = (y3.v[q] & sum) | (ly.v[q] & lift) | (acc.Y.v[q] & keep);
    acc.Z.v[q] = (z3.v[q] & sum) | (one.v[q] & lift) | (acc.Z.v[q] & keep);
  }
  acc_inf &= digit_zero;
}

// [kp]G for 0 < kp < 2^255, affine x as plain little-endian words (and y when wanted):
// 64 branch-free additions from the top digit down, then one inversion
template <class C, bool kWantY>
CDEV void ec_sign_comb_mult(u256& xo, u256& yo, const uint32_t kp[8], const uint32_t* __restrict__ comb) {
  using F = typename C::F;
  uint32_t enc[8];
  ecs_recode(enc, kp);
  jpt acc;
  f29_const_one<F>(acc.X);
  f29_const_one<F>(acc.Y);
  f29_const_one<F>(acc.Z);
  acc.inf = false;  // unused: the flag below is the state
  uint32_t inf = ct_mask(true);
#pragma unroll 1
  for (int j = kCombDigits - 1; j >= 0; j--) {
    const int d = (int)(enc[7] >> 28) - 7;  // digit j, then the next one moves up
#pragma unroll
    for (int q = 7; q > 0; q--) enc[q] = (enc[q] << 4) | (enc[q - 1] >> 28);
    enc[0] <<= 4;
    f29 x, y;
    ec_sign_select<F>(x, y, comb, j, d);
    jmadd_ct<C>(acc, inf, x, y, ct_mask(d == 0));
  }
  // kp != 0 (mod n): the sum is a finite point, Z != 0
  f29 zi, zi2, X;
  f29_pow_const<F, typename C::Pm2>(zi, acc.Z);
  f29_sqr<F>(zi2, zi);
  f29_mul<F>(X, acc.X, zi2);
  f29_from_mont<F>(X, X);
  f29_to_words(xo.v, X);
  if constexpr (kWantY) {
    f29 Y;
    f29_mul<F>(zi2, zi2, zi);
    f29_mul<F>(Y, acc.Y, zi2);
    f29_from_mont<F>(Y, Y);
    f29_to_words(yo.v, Y);
  }
}

// ---------------------------------------------------------------------------
// A key added: one lane. d comes through the table's scratch words, which this
// kernel zeroes before anything else. d = 0 or d >= n: nothing is written but the
// answer word (0). Else the record of `slot` and, in the scratch, 1 and Q = [d]G.
template <class C, int S>
__global__ void __launch_bounds__(64) ecdsa_signer_add_kernel(uint32_t* __restrict__ tab, uint32_t slot,
                                                              uint32_t key_id) {
  using N = typename C::N;
  if (blockIdx.x || threadIdx.x) return;
  uint32_t* key = tab + kEcSignKeyWord;
  uint32_t* out = tab + kEcSignOutWord;
  u256 d;
#pragma unroll
  for (int q = 0; q < 8; q++) d.v[7 - q] = bswap32(key[q]);
#pragma unroll
  for (int q = 0; q < 8; q++) key[q] = 0;
  const u256 nm = mod_m<N>();
  const bool ok = !u256_iszero(d) && !u256_geq(d, nm);  // whether d is a key is the caller's answer: public
  out[0] = ok ? 1u : 0u;
  if (!ok) return;
  uint32_t dp[8];
  const uint32_t flip = ecs_split_min(dp, d.v, nm.v);
  u256 qx, qy, t;
  ec_sign_comb_mult<C, true>(qx, qy, dp, tab + ec_sign_comb_base(S));
  u256_sub(t, mod_m<typename C::P>(), qy);  // y != 0 on a curve of odd order
  const uint32_t fm = ct_mask(flip != 0);
#pragma unroll
  for (int q = 0; q < 8; q++) qy.v[q] = ct_sel(fm, t.v[q], qy.v[q]);
  uint32_t* rec = tab + kEcSignRecBase + slot * kEcSignRecWords;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    rec[kEcSignRecD + q] = d.v[q];
    const uint32_t xw = bswap32(qx.v[7 - q]), yw = bswap32(qy.v[7 - q]);  // big-endian bytes
    rec[kEcSignRecPub + q] = xw;
    rec[kEcSignRecPub + 8 + q] = yw;
    out[4 + q] = xw;
    out[12 + q] = yw;
  }
  rec[kEcSignRecScheme] = (uint32_t)S;
  rec[kEcSignRecId] = key_id;
  rec[kEcSignRecLive] = 1u;
}

// ---------------------------------------------------------------------------
// K17, one instance per curve; a call launches the instance of every curve that has a
// live signer key on the device (the P-256 one when none has: it then only writes
// SKIPPED and UNKNOWN_KEY). Messages: moff / mlen non-null: lane i's message is
// mlen[i] bytes at msgs + moff[i]; else dense rows of msg_len bytes. Statuses by
// precedence: SKIPPED (gate[i] != 0), UNKNOWN_KEY (the record of the id's slot holds
// another id, or none), EMPTY (no message byte), SIGN_FAILED (kEcSignMaxTries
// candidates rejected), OK. A lane that is not OK writes a zero row and length 0 and
// reads nothing but its record's id, live and scheme words. A lane whose key is of the
// other curve is left to that curve's instance.
template <int S>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) ecdsa_sign_keyed_kernel(
    const uint32_t* __restrict__ key_id, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ moff,
    const uint32_t* __restrict__ mlen, uint32_t msg_len, uint64_t n, const uint8_t* __restrict__ gate,
    const uint32_t* __restrict__ tab, uint8_t* __restrict__ sigs, uint8_t* __restrict__ sig_len,
    uint8_t* __restrict__ status) {
  using C = Curve<S>;
  using N = typename C::N;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = key_id[i];
  const uint32_t len = moff ? mlen[i] : msg_len;
  const uint8_t* msg = moff ? msgs + moff[i] : msgs + i * (uint64_t)msg_len;
  const uint32_t* rec = tab + kEcSignRecBase + (uint64_t)(id & (kSignKeySlots - 1)) * kEcSignRecWords;
  uint8_t st = kStatusOk;
  if (gate && gate[i]) st = kSignSkipped;
  else if (!tab || rec[kEcSignRecId] != id || rec[kEcSignRecLive] != 1u) st = kSignUnknownKey;
  else if (rec[kEcSignRecScheme] != (uint32_t)S) return;  // the other curve's instance decides
  else if (len == 0) st = kStatusEmpty;
  uint32_t* row = reinterpret_cast<uint32_t*>(sigs + i * kEcSignSigBytes);
  uint32_t ow[kEcSignSigBytes / 4];
#pragma unroll
  for (int q = 0; q < (int)kEcSignSigBytes / 4; q++) ow[q] = 0;
  uint32_t olen = 0;
  if (st == kStatusOk) {
    const u256 nm = mod_m<N>();
    u256 d, e;
#pragma unroll
    for (int q = 0; q < 8; q++) d.v[q] = rec[kEcSignRecD + q];
    {
      uint32_t hw[8];
      sha256_bytes(hw, msg, len);
      u256 h;
#pragma unroll
      for (int q = 0; q < 8; q++) h.v[q] = hw[7 - q];
      ecs_reduce_once(e.v, h.v, nm.v);  // e = int(h1) mod n = bits2octets(h1)
    }
    ecs_drbg g;
    {
      ecs_w8 xb, hb;
#pragma unroll
      for (int q = 0; q < 8; q++) {
        xb.v[q] = d.v[7 - q];
        hb.v[q] = e.v[7 - q];
      }
      ecs_drbg_init(g, xb, hb);
    }
    u256 dm;
    to_mont<N>(dm, d);
    st = kSignFailed;
    u256 k;
#pragma unroll 1
    while (ecs_next_nonce(g, k.v, nm.v, kEcSignMaxTries)) {
      uint32_t kp[8];
      const uint32_t flip = ecs_split_min(kp, k.v, nm.v);
      u256 x, unused, r, s;
      ec_sign_comb_mult<C, false>(x, unused, kp, tab + ec_sign_comb_base(S));
      ecs_reduce_once(r.v, x.v, nm.v);  // x < p < 2n
      // s = k^-1 (e + d r): k'^-1 by the fixed chain, negated by select when k = n - k'
      u256 kpv, km, kinv, kneg, rd, sum;
#pragma unroll
      for (int q = 0; q < 8; q++) kpv.v[q] = kp[q];
      to_mont<N>(km, kpv);
      mont_pow_const<N, typename C::Nm2>(kinv, km);  // Montgomery form, non-zero
      u256_sub(kneg, nm, kinv);
      const uint32_t fm = ct_mask(flip != 0);
#pragma unroll
      for (int q = 0; q < 8; q++) kinv.v[q] = ct_sel(fm, kneg.v[q], kinv.v[q]);
      mont_mul<N>(rd, dm, r);  // plain d r (the Montgomery factor of dm cancels)
      mod_add<N>(sum, e, rd);
      mont_mul<N>(s, kinv, sum);  // plain
      if (u256_iszero(r) || u256_iszero(s)) continue;  // the candidate is discarded
      uint8_t body[70];
      uint32_t p = der_put_int(body, r);
      p += der_put_int(body + p, s);
      olen = p + 2;
      ow[0] = 0x30u | (p << 8);
      for (uint32_t b = 0; b < p; b++) ow[(b + 2) >> 2] |= (uint32_t)body[b] << (8 * ((b + 2) & 3));
      st = kStatusOk;
      break;
    }
    if (st != kStatusOk) {
#pragma unroll
      for (int q = 0; q < (int)kEcSignSigBytes / 4; q++) ow[q] = 0;
      olen = 0;
    }
  }
#pragma unroll
  for (int q = 0; q < (int)kEcSignSigBytes / 4; q++) row[q] = ow[q];
  sig_len[i] = (uint8_t)olen;
  status[i] = st;
}

// ---------------------------------------------------------------------------
// host-side launchers (called by keyed.cpp)
size_t ecdsa_signtab_bytes() { return (size_t)kEcSignAllWords * sizeof(uint32_t); }

hipError_t launch_ecdsa_sign_comb(uint32_t* tab, uint32_t scheme, hipStream_t s) {
  const dim3 g(kCombDigits * kCombEntries / 64);
  if (scheme == 2) hipLaunchKernelGGL(ecdsa_sign_comb_kernel<Curve<2>>, g, dim3(64), 0, s, tab + ec_sign_comb_base(2));
  else hipLaunchKernelGGL(ecdsa_sign_comb_kernel<Curve<3>>, g, dim3(64), 0, s, tab + ec_sign_comb_base(3));
  return hipGetLastError();
}

hipError_t launch_ecdsa_signer_add(uint32_t* tab, uint32_t scheme, uint32_t key_id, hipStream_t s) {
  const uint32_t slot = key_id & (kSignKeySlots - 1);
  if (scheme == 2) hipLaunchKernelGGL((ecdsa_signer_add_kernel<Curve<2>, 2>), dim3(1), dim3(64), 0, s, tab, slot, key_id);
  else hipLaunchKernelGGL((ecdsa_signer_add_kernel<Curve<3>, 3>), dim3(1), dim3(64), 0, s, tab, slot, key_id);
  return hipGetLastError();
}

// live_k1 / live_r1: whether the device holds a live signer key of that curve
hipError_t launch_ecdsa_sign_keyed(const uint32_t* key_id, const uint8_t* msgs, const uint64_t* moff,
                                   const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* gate,
                                   const uint32_t* tab, bool live_k1, bool live_r1, uint8_t* sigs, uint8_t* sig_len,
                                   uint8_t* status, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)blocks);
  if (live_k1)
    hipLaunchKernelGGL(ecdsa_sign_keyed_kernel<2>, grid, dim3(256), 0, s, key_id, msgs, moff, mlen, msg_len, n, gate,
                       tab, sigs, sig_len, status);
  if (live_r1 || !live_k1)
    hipLaunchKernelGGL(ecdsa_sign_keyed_kernel<3>, grid, dim3(256), 0, s, key_id, msgs, moff, mlen, msg_len, n, gate,
                       tab, sigs, sig_len, status);
  return hipGetLastError();
}
