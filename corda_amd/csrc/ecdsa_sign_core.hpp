// The scalar side of ECDSA signing with registered keys (kernel K17,
// ecdsa_sign_keyed.hip): the RFC 6979 nonce, the split k' = min(k, n - k), the
// signed 4-bit recoding of k', and the layout of the signer's table. Usable from
// host and device (tests/test_ecdsa_sign_core.py builds tools/ecdsa_sign_check.cpp
// from it); the modulus and the try bound are parameters, so a host program runs
// the retry path with a modulus that rejects half of all candidates.
//
// Nonce (RFC 6979 3.2, HMAC-SHA256, qlen = 256 on both curves): x = int2octets(d),
// h1' = bits2octets(SHA-256(m)) = int(h1) mod n as 32 bytes;
//   K = 00..00, V = 01..01
//   K = HMAC_K(V || 00 || x || h1'), V = HMAC_K(V)
//   K = HMAC_K(V || 01 || x || h1'), V = HMAC_K(V)
//   candidate: V = HMAC_K(V), k = int(V); rejected (k = 0, k >= n, or, by the
//   caller, r = 0 or s = 0): K = HMAC_K(V || 00), V = HMAC_K(V), next candidate.
// Every HMAC message has a fixed length (97, 32 or 33 bytes), every block is
// assembled with shifts of whole words, and a key's inner and outer pad states are
// computed once per K: 18 compressions up to the first candidate. Nothing here
// indexes memory by, or branches on, x, h1', K or V; the only data-dependent branch
// is the verdict on a candidate, which is discarded when it is rejected.
//
// Split: k' = min(k, n - k) by select; k' <= (n - 1) / 2 < 2^255, and
// x([k']G) = x([k]G). Recoding: k' = sum_j d_j 16^j with d_j in [-7, 8]
// (ed25519_comb.hpp comb_step); nibble 63 of k' < 2^255 is at most 7, so digit 63
// is at most 8 and no carry leaves it. The digits are kept as nibbles d_j + 7 of
// eight words, so that the kernel can take them from the top by shifting.
#pragma once
#include <stdint.h>

#include "ed25519_comb.hpp"

namespace cordahip {

// ---- the signer's table of one device ---------------------------------------
// Two comb tables [d 16^j]G, d = 1..8, j = 0..63 (secp256k1, then P-256; entries
// affine, canonical, Montgomery form, the 20-word layout of ecdsa.hip's load_g:
// 40 KiB each), then kSignKeySlots records of 32 words -- d (8 little-endian words),
// Q as X || Y (64 big-endian bytes), the key id, a live word, the scheme -- then the
// scratch the add kernel takes d from (32 big-endian bytes, zeroed by the kernel)
// and leaves its answer in (word 0: 1 = key taken, then Q at word 4). Ids and slots
// are the Ed25519 signer's (one pool); a slot's record here is zero while the slot
// holds an Ed25519 key, and the other way round.
static constexpr int kEcSignEntryWords = 20;
static constexpr uint32_t kEcSignCombWords = kCombDigits * kCombEntries * kEcSignEntryWords;  // 40 KiB
static_assert(kEcSignCombWords * 4u == 40u * 1024u, "a curve's comb table is 40 KiB");
static constexpr uint32_t kEcSignRecBase = 2 * kEcSignCombWords;
static constexpr int kEcSignRecWords = 32;
static constexpr int kEcSignRecD = 0, kEcSignRecPub = 8, kEcSignRecId = 24, kEcSignRecLive = 25, kEcSignRecScheme = 26;
static constexpr uint32_t kEcSignKeyWord = kEcSignRecBase + kSignKeySlots * kEcSignRecWords;  // 8 words in
static constexpr uint32_t kEcSignOutWord = kEcSignKeyWord + 8;                                // 20 words out
static constexpr uint32_t kEcSignAllWords = kEcSignOutWord + 20;
static constexpr uint32_t kEcSignMaxTries = 8;  // candidates per lane before SIGN_FAILED
static constexpr uint32_t kEcSignSigBytes = 72;

COMB_HD constexpr uint32_t ec_sign_comb_base(uint32_t scheme) { return scheme == 2 ? 0u : kEcSignCombWords; }
// word offset, within a comb table, of the entry [d 16^j]G, d = 1..8
COMB_HD constexpr uint32_t ec_sign_entry_word(int j, int d) {
  return (uint32_t)comb_index(j, d) * kEcSignEntryWords;
}

// ---- SHA-256 compression, by value (on the device: one function, called) ------
struct ecs_w8 {
  uint32_t v[8];
};
struct ecs_w16 {
  uint32_t v[16];
};

#if defined(__HIPCC__)
#define ECS_FN __host__ __device__ __attribute__((noinline)) inline
#else
#define ECS_FN __attribute__((noinline)) inline
#endif

COMB_HD uint32_t ecs_ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

ECS_FN ecs_w8 ecs_sha256_compress(ecs_w8 h, ecs_w16 w) {
  const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
      0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
      0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
      0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
      0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t a = h.v[0], b = h.v[1], c = h.v[2], d = h.v[3], e = h.v[4], f = h.v[5], g = h.v[6], hh = h.v[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    uint32_t wi;
    if (i < 16) {
      wi = w.v[i];
    } else {
      const uint32_t w15 = w.v[(i - 15) & 15], w2 = w.v[(i - 2) & 15];
      const uint32_t s0 = ecs_ror(w15, 7) ^ ecs_ror(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = ecs_ror(w2, 17) ^ ecs_ror(w2, 19) ^ (w2 >> 10);
      wi = w.v[i & 15] + s0 + w.v[(i - 7) & 15] + s1;
      w.v[i & 15] = wi;
    }
    const uint32_t t1 = hh + (ecs_ror(e, 6) ^ ecs_ror(e, 11) ^ ecs_ror(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + wi;
    const uint32_t t2 = (ecs_ror(a, 2) ^ ecs_ror(a, 13) ^ ecs_ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h.v[0] += a; h.v[1] += b; h.v[2] += c; h.v[3] += d; h.v[4] += e; h.v[5] += f; h.v[6] += g; h.v[7] += hh;
  return h;
}

COMB_HD ecs_w8 ecs_sha256_iv() {
  return ecs_w8{{0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu,
                 0x5be0cd19u}};
}

// ---- HMAC-SHA256 with a 32-byte key (words big-endian, as SHA-256 reads them) ---
struct ecs_hmac_key {
  ecs_w8 in, out;  // the states after the key's inner and outer pad blocks
};

COMB_HD ecs_hmac_key ecs_hmac_pads(const ecs_w8& key) {
  ecs_w16 bi, bo;
  for (int i = 0; i < 16; i++) {
    const uint32_t kw = i < 8 ? key.v[i] : 0u;
    bi.v[i] = kw ^ 0x36363636u;
    bo.v[i] = kw ^ 0x5c5c5c5cu;
  }
  ecs_hmac_key hk;
  hk.in = ecs_sha256_compress(ecs_sha256_iv(), bi);
  hk.out = ecs_sha256_compress(ecs_sha256_iv(), bo);
  return hk;
}

// the outer hash over the 32-byte inner digest
COMB_HD ecs_w8 ecs_hmac_outer(const ecs_hmac_key& hk, const ecs_w8& inner) {
  ecs_w16 b;
  for (int i = 0; i < 8; i++) b.v[i] = inner.v[i];
  b.v[8] = 0x80000000u;
  for (int i = 9; i < 15; i++) b.v[i] = 0;
  b.v[15] = (64 + 32) * 8;
  return ecs_sha256_compress(hk.out, b);
}

// HMAC_K(V) (tail false) or HMAC_K(V || 00) (tail true): one inner block
COMB_HD ecs_w8 ecs_hmac_v(const ecs_hmac_key& hk, const ecs_w8& V, bool tail) {
  ecs_w16 b;
  for (int i = 0; i < 8; i++) b.v[i] = V.v[i];
  b.v[8] = tail ? 0x00800000u : 0x80000000u;
  for (int i = 9; i < 15; i++) b.v[i] = 0;
  b.v[15] = (64 + 32 + (tail ? 1 : 0)) * 8;
  return ecs_hmac_outer(hk, ecs_sha256_compress(hk.in, b));
}

// HMAC_K(V || sep || x || h1): 97 bytes, two inner blocks; sep is 0 or 1
COMB_HD ecs_w8 ecs_hmac_vxh(const ecs_hmac_key& hk, const ecs_w8& V, uint32_t sep, const ecs_w8& x, const ecs_w8& h1) {
  uint32_t s[16], o[17];
  for (int i = 0; i < 8; i++) {
    s[i] = x.v[i];
    s[8 + i] = h1.v[i];
  }
  // the 64 bytes of x || h1 moved one byte down the stream, behind sep
  o[0] = (sep << 24) | (s[0] >> 8);
  for (int i = 1; i < 16; i++) o[i] = (s[i - 1] << 24) | (s[i] >> 8);
  o[16] = (s[15] << 24) | 0x00800000u;
  ecs_w16 b;
  for (int i = 0; i < 8; i++) {
    b.v[i] = V.v[i];
    b.v[8 + i] = o[i];
  }
  const ecs_w8 mid = ecs_sha256_compress(hk.in, b);
  for (int i = 0; i < 9; i++) b.v[i] = o[8 + i];
  for (int i = 9; i < 15; i++) b.v[i] = 0;
  b.v[15] = (64 + 97) * 8;
  return ecs_hmac_outer(hk, ecs_sha256_compress(mid, b));
}

// ---- the nonce generator ------------------------------------------------------
struct ecs_drbg {
  ecs_w8 V;
  ecs_hmac_key hk;  // the pad states of the current K (K itself is not needed again)
  uint32_t tries;   // candidates drawn so far
};

// x: the private key, h1: int(SHA-256(m)) mod n, both as 8 big-endian words
COMB_HD void ecs_drbg_init(ecs_drbg& st, const ecs_w8& x, const ecs_w8& h1) {
  ecs_w8 K, V;
  for (int i = 0; i < 8; i++) {
    K.v[i] = 0;
    V.v[i] = 0x01010101u;
  }
  ecs_hmac_key hk = ecs_hmac_pads(K);
  for (uint32_t sep = 0; sep < 2; sep++) {
    K = ecs_hmac_vxh(hk, V, sep, x, h1);
    hk = ecs_hmac_pads(K);
    V = ecs_hmac_v(hk, V, false);
  }
  st.V = V;
  st.hk = hk;
  st.tries = 0;
}

// The next candidate in [1, n - 1] as little-endian words; false once `bound`
// candidates have been drawn. A caller that rejects the nonce it got (r = 0 or
// s = 0) calls again: the 3.2 h.3 update runs before every candidate but the first.
COMB_HD bool ecs_next_nonce(ecs_drbg& st, uint32_t k[8], const uint32_t n[8], uint32_t bound) {
  while (st.tries < bound) {
    if (st.tries) {
      const ecs_w8 K = ecs_hmac_v(st.hk, st.V, true);
      st.hk = ecs_hmac_pads(K);
      st.V = ecs_hmac_v(st.hk, st.V, false);
    }
    st.tries++;
    st.V = ecs_hmac_v(st.hk, st.V, false);
    uint32_t nz = 0, br = 0;
    for (int i = 0; i < 8; i++) {
      k[i] = st.V.v[7 - i];
      nz |= k[i];
      br = (uint32_t)(((uint64_t)k[i] - n[i] - br) >> 63);  // borrow of k - n
    }
    if (nz != 0 && br != 0) return true;
  }
  return false;
}

// a mod n for a < 2n (little-endian words), by select: bits2octets' reduction of h1
// (n > 2^255 on both curves) and r = x mod n
COMB_HD void ecs_reduce_once(uint32_t out[8], const uint32_t a[8], const uint32_t n[8]) {
  uint32_t t[8];
  uint64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)a[i] - n[i] - br;
    t[i] = (uint32_t)d;
    br = (d >> 63) & 1u;
  }
  const uint32_t m = 0u - (uint32_t)br;  // all ones: a < n, keep a
  for (int i = 0; i < 8; i++) out[i] = (a[i] & m) | (t[i] & ~m);
}

// ---- k' = min(k, n - k) and its digits ------------------------------------------
// 0 < k < n. Returns 1 when k' = n - k (then [k]G = -[k']G and k^-1 = -(k'^-1)).
COMB_HD uint32_t ecs_split_min(uint32_t out[8], const uint32_t k[8], const uint32_t n[8]) {
  uint32_t t[8];
  uint64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)n[i] - k[i] - br;
    t[i] = (uint32_t)d;
    br = (d >> 63) & 1u;
  }
  uint32_t lt = 0;  // borrow of t - k: n - k < k
  for (int i = 0; i < 8; i++) lt = (uint32_t)(((uint64_t)t[i] - k[i] - lt) >> 63);
  const uint32_t m = 0u - lt;
  for (int i = 0; i < 8; i++) out[i] = (t[i] & m) | (k[i] & ~m);
  return lt;
}

// nibble j of enc = d_j + 7; returns the carry out of digit 63 (0 for k' < 2^255)
COMB_HD uint32_t ecs_recode(uint32_t enc[8], const uint32_t kp[8]) {
  uint32_t carry = 0;
  for (int q = 0; q < 8; q++) {
    uint32_t e = 0;
    for (int t = 0; t < 8; t++) {
      const int d = comb_step((kp[q] >> (4 * t)) & 15u, carry);
      e |= (uint32_t)(d + 7) << (4 * t);
    }
    enc[q] = e;
  }
  return carry;
}
COMB_HD int ecs_digit(const uint32_t enc[8], int j) { return (int)((enc[j >> 3] >> (4 * (j & 7))) & 15u) - 7; }

}  // namespace cordahip
