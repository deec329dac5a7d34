// Ed25519 (EDDSA_ED25519_SHA512) batch signing with registered keys for gfx950
// -- kernel K11.
//
// Replaces, per lane, the reference's
//   Crypto.doSign(EDDSA_ED25519_SHA512, privateKey, clearData)   Crypto.kt:394-401
//   -> i2p eddsa 0.2.0 EdDSAEngine.engineSign (RFC 8032 5.1.6, deterministic)
// for a handful of long-lived keys and many messages: a key is expanded once
// (ed25519_key_expand_kernel: h = SHA-512(seed), a = clamp(h[0:32]) mod L,
// prefix = h[32:64], A = [a]B) into a 128-byte record of the device's key
// table; a lane then needs
//   r = SHA-512(prefix || M) mod L,  R = [r]B,
//   k = SHA-512(R || A || M) mod L,  S = (r + k a) mod L.
// [r]B is 64 mixed additions from the comb table [d 16^j]B (d = 1..8,
// j = 0..63, 64 KB, built once per device): no doublings.
//
// Secrets are the seed, a, the prefix, r and r's digits. No address and no
// branch depends on them: for position j every lane reads all 8 entries of
// that position (addresses depend on j alone), picks its own by compare and
// select, negates by select (comb_select); the digits come from arithmetic on
// r (ed25519_comb.hpp); the reductions mod L end in selects
// (sc_reduce512<true>); the field inversion is a fixed square-and-multiply
// chain. What does branch is public: the lane's status (gate byte, key id,
// message length) and the message length in SHA-512's block loop.
// Oracle: oracle/i2p_ed25519.py sign, oracle/c oracle_ed25519_sign.
#ifndef FE_QUAD
#define FE_QUAD 0
#endif
#ifndef FE_USE_ASM2
#define FE_USE_ASM2 1
#endif
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ed25519_comb.hpp"
#include "ed25519_ops.hpp"
#include "status.hpp"

namespace cordahip {

// ---------------------------------------------------------------------------
// comb table: entry comb_index(j, d) = [d 16^j]B as affine niels
__global__ void __launch_bounds__(64) ed25519_comb_kernel(uint32_t* __restrict__ tab) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= kCombDigits * kCombEntries) return;
  const int j = g / kCombEntries, d = g % kCombEntries + 1;
  ge_p3 P, Q;
  ge_base(P);
  for (int t = 0; t < 4 * j; t++) ge_dbl<true>(P, P);
  ge_cached pc;
  ge_to_cached(pc, P);
  ge_identity(Q);
  for (int e = 0; e < d; e++) ge_add<true>(Q, Q, pc);
  store_niels_entry(tab + g * kCombEntryWords, Q);
}

// the entry of position j for the digit d in [-8, 8]: every entry of the
// position is read, the lane's own kept by select; d == 0 keeps the identity
CDEV void comb_select(ge_niels& n, const uint32_t* __restrict__ comb, int j, int d) {
  const int sgn = d >> 31;  // 0 or -1
  const uint32_t ad = (uint32_t)((d ^ sgn) - sgn);
  fe_set(n.ypx, 1);
  fe_set(n.ymx, 1);
  fe_set(n.xy2d, 0);
#pragma unroll
  for (int e = 1; e <= kCombEntries; e++) {
    ge_niels t;
    load_niels(t, comb, comb_index(j, e));
    const bool hit = ad == (uint32_t)e;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      n.ypx.v[i] = hit ? t.ypx.v[i] : n.ypx.v[i];
      n.ymx.v[i] = hit ? t.ymx.v[i] : n.ymx.v[i];
      n.xy2d.v[i] = hit ? t.xy2d.v[i] : n.xy2d.v[i];
    }
  }
  niels_cneg(n, sgn != 0);
}

// P = [k]B for k < 2^253: 64 mixed additions, one per signed digit of k
CDEV void comb_mult(ge_p3& P, const uint32_t k[8], const uint32_t* __restrict__ comb) {
  uint32_t w[8];
#pragma unroll
  for (int q = 0; q < 8; q++) w[q] = k[q];
  uint32_t carry = 0;
  ge_identity(P);
#pragma unroll 1
  for (int j = 0; j < kCombDigits; j++) {
    const int d = comb_step(w[0] & 15u, carry);
#pragma unroll
    for (int q = 0; q < 7; q++) w[q] = (w[q] >> 4) | (w[q + 1] << 28);
    w[7] >>= 4;
    ge_niels n;
    comb_select(n, comb, j, d);
    ge_madd<true>(P, P, n);
  }
}

// SHA-512(prefix || M) for a 32-byte, 16-byte-aligned M: one block
CDEV void sha512_prefix_msg32(uint32_t out_le[16], const uint32_t s0[8], const uint8_t* __restrict__ msg) {
  uint64_t h[8], w[16];
  sha512_init(h);
  uint32_t m[8];
  load8(m, reinterpret_cast<const uint32_t*>(msg));
#pragma unroll
  for (int q = 0; q < 4; q++) {
    w[q] = ((uint64_t)bswap32(s0[2 * q]) << 32) | bswap32(s0[2 * q + 1]);
    w[4 + q] = ((uint64_t)bswap32(m[2 * q]) << 32) | bswap32(m[2 * q + 1]);
  }
  w[8] = 0x8000000000000000ULL;
#pragma unroll
  for (int q = 9; q < 15; q++) w[q] = 0;
  w[15] = 64 * 8;
  sha512_block(h, w);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out_le[2 * i] = bswap32((uint32_t)(h[i] >> 32));
    out_le[2 * i + 1] = bswap32((uint32_t)h[i]);
  }
}

// ---------------------------------------------------------------------------
// key expansion: one lane. The seed comes through the table's scratch words,
// which this kernel zeroes before anything else.
__global__ void __launch_bounds__(64) ed25519_key_expand_kernel(uint32_t* __restrict__ keytab, uint32_t slot,
                                                                uint32_t key_id, const uint32_t* __restrict__ comb) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t seed[8], zero[8];
  load8(seed, keytab + kSignSeedWord);
#pragma unroll
  for (int q = 0; q < 8; q++) zero[q] = 0;
  store8(keytab + kSignSeedWord, zero);
  uint32_t hs[16];
  sha512_segments(hs, seed, zero, false, nullptr, 0);
  uint32_t a16[16], prefix[8], ar[8];
#pragma unroll
  for (int q = 0; q < 8; q++) {
    a16[q] = hs[q];
    a16[8 + q] = 0;
    prefix[q] = hs[8 + q];
  }
  a16[0] &= ~7u;
  a16[7] &= 0x3fffffffu;
  a16[7] |= 0x40000000u;
  sc_reduce512<true>(ar, a16);
  ge_p3 A;
  comb_mult(A, ar, comb);
  uint32_t pub[8];
  ge_tobytes(pub, A);
  uint32_t* rec = keytab + slot * kSignRecWords;
  store8(rec + kSignRecA, ar);
  store8(rec + kSignRecPrefix, prefix);
  store8(rec + kSignRecPub, pub);
  uint32_t tail[8] = {key_id, 1u, 0u, 0u, 0u, 0u, 0u, 0u};
  store8(rec + kSignRecId, tail);
  store8(keytab + kSignPubWord, pub);
}

// ---------------------------------------------------------------------------
// K11. Messages: moff / mlen non-null: lane i's message is mlen[i] bytes at
// msgs + moff[i] (16-byte aligned starts); else dense rows of msg_len bytes.
// Statuses by precedence: SKIPPED (gate[i] != 0), UNKNOWN_KEY (the record of
// the id's slot holds another id, or none), EMPTY (no message byte). Such a
// lane writes a zero row and reads nothing but its record's id and live words.
__global__ void __launch_bounds__(256) ed25519_sign_keyed_kernel(
    const uint32_t* __restrict__ key_id, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ moff,
    const uint32_t* __restrict__ mlen, uint32_t msg_len, uint64_t n, const uint8_t* __restrict__ gate,
    const uint32_t* __restrict__ keytab, const uint32_t* __restrict__ comb, uint8_t* __restrict__ sigs,
    uint8_t* __restrict__ status) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = key_id[i];
  const uint32_t len = moff ? mlen[i] : msg_len;
  const uint8_t* msg = moff ? msgs + moff[i] : msgs + i * (uint64_t)msg_len;
  const uint32_t* rec = keytab + (uint64_t)(id & (kSignKeySlots - 1)) * kSignRecWords;
  uint8_t st = kStatusOk;
  if (gate && gate[i]) st = kSignSkipped;
  else if (!keytab || rec[kSignRecId] != id || rec[kSignRecLive] != 1u) st = kSignUnknownKey;
  else if (len == 0) st = kStatusEmpty;
  uint4* s4 = reinterpret_cast<uint4*>(sigs + i * 64);
  status[i] = st;
  if (st != kStatusOk) {
    s4[0] = s4[1] = s4[2] = s4[3] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  uint32_t a[8], prefix[8], pub[8];
  load8(a, rec + kSignRecA);
  load8(prefix, rec + kSignRecPrefix);
  load8(pub, rec + kSignRecPub);
  uint32_t rh[16], r[8], dummy[8];
#pragma unroll
  for (int q = 0; q < 8; q++) dummy[q] = 0;
  if (len == 32) sha512_prefix_msg32(rh, prefix, msg);
  else sha512_segments(rh, prefix, dummy, false, msg, len);
  sc_reduce512<true>(r, rh);
  ge_p3 Rp;
  comb_mult(Rp, r, comb);
  uint32_t R[8];
  ge_tobytes(R, Rp);
  uint32_t kh[16], k[8], S[8];
  sha512_segments(kh, R, pub, true, msg, len);
  sc_reduce512<true>(k, kh);
  sc_muladd<true>(S, k, a, r);
  s4[0] = make_uint4(R[0], R[1], R[2], R[3]);
  s4[1] = make_uint4(R[4], R[5], R[6], R[7]);
  s4[2] = make_uint4(S[0], S[1], S[2], S[3]);
  s4[3] = make_uint4(S[4], S[5], S[6], S[7]);
}

// ---------------------------------------------------------------------------
// host-side launchers (called by runtime.cpp / cordahip.cpp / host_batch.cpp)
size_t ed25519_comb_bytes() { return (size_t)kCombTableWords * sizeof(uint32_t); }
size_t ed25519_keytab_bytes() { return (size_t)kSignTableWords * sizeof(uint32_t); }

hipError_t launch_ed25519_comb(uint32_t* tab, hipStream_t s) {
  hipLaunchKernelGGL(ed25519_comb_kernel, dim3(kCombDigits * kCombEntries / 64), dim3(64), 0, s, tab);
  return hipGetLastError();
}

hipError_t launch_ed25519_key_expand(uint32_t* keytab, uint32_t key_id, const uint32_t* comb, hipStream_t s) {
  hipLaunchKernelGGL(ed25519_key_expand_kernel, dim3(1), dim3(64), 0, s, keytab, key_id & (kSignKeySlots - 1), key_id,
                     comb);
  return hipGetLastError();
}

hipError_t launch_ed25519_sign_keyed(const uint32_t* key_id, const uint8_t* msgs, const uint64_t* moff,
                                     const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* gate,
                                     const uint32_t* keytab, const uint32_t* comb, uint8_t* sigs, uint8_t* status,
                                     hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ed25519_sign_keyed_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, key_id, msgs, moff, mlen,
                     msg_len, n, gate, keytab, comb, sigs, status);
  return hipGetLastError();
}

}  // namespace cordahip
