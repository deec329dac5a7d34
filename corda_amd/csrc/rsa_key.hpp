// RSA_SHA256 (Crypto.kt:77-88, "SHA256WITHRSAANDMGF1" = RSASSA-PSS, SHA-256,
// MGF1-SHA-256, salt 32, trailer 0xBC) on the host: the strict DER parser of the
// key's wire form (the SPKI BIT STRING payload, RSAPublicKey ::= SEQUENCE {
// modulus INTEGER, publicExponent INTEGER }), the width-class rule of the GPU
// path, and a simple word-serial reference of the whole verification
// (Montgomery CIOS, SHA-256, the PSS rules of BouncyCastle 1.57's
// PSSSigner.verifySignature as DESIGN §5 restates them; PARITY UNPINNED).
// The generic batch classifies and packs RSA lanes with it (pack_rows.hpp,
// host_batch.cpp); the CPU tests check the GPU kernels' rules against it.
// Plain C++, no HIP: compiles with g++ like der.hpp.
#pragma once
#include <stdint.h>

#include <cstring>
#include <vector>

#include "der.hpp"

namespace cordahip {
namespace rsa {

constexpr uint32_t kMaxWords = 128;  // 4096 bits
constexpr uint32_t kMinBits = 1024, kMaxBits = 4096;

// lane outcomes of key decoding (the values are CORDAHIP_STATUS_*)
constexpr uint8_t kOk = 0, kBadSig = 1, kBadKey = 3, kUnsupported = 4, kEmpty = 5;

struct PublicKey {
  uint32_t n[kMaxWords];  // little-endian words, zero above the modulus
  uint32_t e = 0;
  uint32_t bits = 0;   // bit length of the modulus
  uint32_t words = 0;  // width class: 64, 96 or 128 (0: none)
};

// Width class of a modulus of `bits` bits: the operand width W (32-bit words) its
// lanes run at; the modulus is zero-padded to W words (Montgomery with
// R = 2^(32 W) holds for every odd n < R). 0: outside 1024..4096 bits.
CHD uint32_t class_words(uint32_t bits) {
  if (bits < kMinBits || bits > kMaxBits) return 0;
  return bits <= 2048 ? 64 : bits <= 3072 ? 96 : 128;
}

// One DER INTEGER at b[i..n): body pointer and length; strict (minimal, non-empty).
CHD bool der_integer(const uint8_t* b, uint32_t n, uint32_t& i, const uint8_t*& body, uint32_t& len) {
  if (i >= n || b[i++] != 0x02) return false;
  if (!der_read_len(b, n, i, len) || len == 0 || len > n - i) return false;
  body = b + i;
  if (len > 1 && ((body[0] == 0 && body[1] < 0x80) || (body[0] == 0xff && body[1] >= 0x80))) return false;
  i += len;
  return true;
}

// A decoded key without a copy of its modulus: the modulus' significant bytes where they
// lie in the key (big-endian, nb[0] != 0), its bit length and width class, and e. What
// the device packer (sig_pack.hpp, K23) keeps of a lane's key: it writes the modulus
// words straight into the lane's row.
struct KeyView {
  const uint8_t* nb = nullptr;
  uint32_t nl = 0;
  uint32_t e = 0;
  uint32_t bits = 0;
  uint32_t words = 0;
};

// word k (little-endian) of the view's modulus, zero above it
CHD uint32_t key_view_word(const KeyView& kv, uint32_t k) {
  uint32_t w = 0;
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t sgn = 4 * k + q;  // significance
    if (sgn < kv.nl) w |= (uint32_t)kv.nb[kv.nl - 1 - sgn] << (8 * q);
  }
  return w;
}

// Decode the key of one lane. kBadKey: not a SEQUENCE of exactly two INTEGERs,
// trailing bytes, non-minimal / indefinite lengths, n <= 0 or e <= 0.
// kUnsupported: a key BouncyCastle accepts and the GPU path declines (even n,
// bit length outside 1024..4096, even e, e < 3, e >= 2^32). kOk: kv is filled.
// Reads der[0 .. len64) only. Host and device: the one rule of both packers.
CHD uint8_t parse_public_key_view(const uint8_t* der, uint64_t len64, KeyView& kv) {
  if (len64 < 2 || len64 > 0xffffffu) return kBadKey;
  const uint32_t n = (uint32_t)len64;
  uint32_t i = 1, len = 0;
  if (der[0] != 0x30 || !der_read_len(der, n, i, len) || len != n - i) return kBadKey;
  const uint8_t *nb = nullptr, *eb = nullptr;
  uint32_t nl = 0, el = 0;
  if (!der_integer(der, n, i, nb, nl) || !der_integer(der, n, i, eb, el) || i != n) return kBadKey;
  if (nb[0] >= 0x80 || eb[0] >= 0x80) return kBadKey;  // negative
  while (nl > 1 && nb[0] == 0) nb++, nl--;
  while (el > 1 && eb[0] == 0) eb++, el--;
  if (nb[0] == 0 || eb[0] == 0) return kBadKey;  // zero
  uint32_t top = nb[0], tb = 0;
  while (top) tb++, top >>= 1;
  const uint64_t bits = (uint64_t)(nl - 1) * 8 + tb;
  if (bits < kMinBits || bits > kMaxBits || !(nb[nl - 1] & 1)) return kUnsupported;
  if (el > 4 || !(eb[el - 1] & 1)) return kUnsupported;
  uint32_t e = 0;
  for (uint32_t k = 0; k < el; k++) e = (e << 8) | eb[k];
  if (e < 3) return kUnsupported;
  kv.nb = nb;
  kv.nl = nl;
  kv.e = e;
  kv.bits = (uint32_t)bits;
  kv.words = class_words(kv.bits);
  return kOk;
}

// a view's key with the modulus materialised
inline void key_of_view(const KeyView& kv, PublicKey& pk) {
  pk.e = kv.e;
  pk.bits = kv.bits;
  pk.words = kv.words;
  std::memset(pk.n, 0, sizeof(pk.n));
  for (uint32_t k = 0; k < kv.nl; k++) pk.n[k >> 2] |= (uint32_t)kv.nb[kv.nl - 1 - k] << (8 * (k & 3));
}
// The same with the modulus materialised (the host packers, the word-serial reference)
inline uint8_t parse_public_key(const uint8_t* der, uint64_t len64, PublicKey& pk) {
  KeyView kv;
  const uint8_t ks = parse_public_key_view(der, len64, kv);
  if (ks == kOk) key_of_view(kv, pk);
  return ks;
}

// big-endian bytes -> w little-endian words; false if the value needs more
inline bool os2ip(const uint8_t* p, uint64_t len, uint32_t* out, uint32_t w) {
  std::memset(out, 0, 4 * (size_t)w);
  for (uint64_t k = 0; k < len; k++) {
    const uint8_t v = p[len - 1 - k];
    if (k >= 4ull * w) {
      if (v) return false;
      continue;
    }
    out[k >> 2] |= (uint32_t)v << (8 * (k & 3));
  }
  return true;
}

inline int cmp_words(const uint32_t* a, const uint32_t* b, uint32_t w) {
  for (uint32_t k = w; k-- > 0;)
    if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
  return 0;
}

inline uint32_t sub_words(uint32_t* a, const uint32_t* b, uint32_t w) {  // a -= b, returns the borrow
  uint64_t br = 0;
  for (uint32_t k = 0; k < w; k++) {
    const uint64_t d = (uint64_t)a[k] - b[k] - br;
    a[k] = (uint32_t)d;
    br = (d >> 32) & 1;
  }
  return (uint32_t)br;
}

// -n^-1 mod 2^32 (n odd): Newton steps, each doubling the correct low bits
inline uint32_t mont_nprime(uint32_t n0) {
  uint32_t x = n0;  // 3 bits
  for (int k = 0; k < 5; k++) x *= 2u - n0 * x;
  return 0u - x;
}

// out = a * b * R^-1 mod n, R = 2^(32 w), a, b < n, n odd; word-serial CIOS
inline void mont_mul(const uint32_t* a, const uint32_t* b, const uint32_t* n, uint32_t np, uint32_t w, uint32_t* out) {
  uint32_t t[kMaxWords + 2];
  std::memset(t, 0, sizeof(t));
  for (uint32_t j = 0; j < w; j++) {
    uint64_t c = 0;
    for (uint32_t i = 0; i < w; i++) {
      const uint64_t u = (uint64_t)a[i] * b[j] + t[i] + c;
      t[i] = (uint32_t)u;
      c = u >> 32;
    }
    uint64_t u = (uint64_t)t[w] + c;
    t[w] = (uint32_t)u;
    t[w + 1] = (uint32_t)(u >> 32);
    const uint32_t q = t[0] * np;
    c = ((uint64_t)q * n[0] + t[0]) >> 32;
    for (uint32_t i = 1; i < w; i++) {
      u = (uint64_t)q * n[i] + t[i] + c;
      t[i - 1] = (uint32_t)u;
      c = u >> 32;
    }
    u = (uint64_t)t[w] + c;
    t[w - 1] = (uint32_t)u;
    t[w] = t[w + 1] + (uint32_t)(u >> 32);
  }
  if (t[w] || cmp_words(t, n, w) >= 0) sub_words(t, n, w);
  std::memcpy(out, t, 4 * (size_t)w);
}

// out = in^e mod n over w-word operands (n odd, in < n, e >= 1): R^2 mod n by
// doubling 2^(bits-1) up to 2^(32 w + s) and squaring in Montgomery form, then
// left-to-right square and multiply -- the same steps as rsa_modexp_kernel.
// Returns false (out = 0) when the operands break the contract.
inline bool modexp(const uint32_t* n, uint32_t e, const uint32_t* in, uint32_t w, uint32_t* out) {
  std::memset(out, 0, 4 * (size_t)w);
  if (w == 0 || w > kMaxWords || !(n[0] & 1) || e == 0 || cmp_words(in, n, w) >= 0) return false;
  uint32_t hi = w;
  while (hi > 0 && n[hi - 1] == 0) hi--;
  uint32_t bits = (hi - 1) * 32;
  for (uint32_t v = n[hi - 1]; v; v >>= 1) bits++;
  uint32_t x[kMaxWords], r2[kMaxWords], acc[kMaxWords], one[kMaxWords];
  std::memset(x, 0, sizeof(x));
  std::memset(one, 0, sizeof(one));
  one[0] = 1;
  if (bits == 1) return true;  // n = 1: everything is 0 mod n (in < n rules it out anyway)
  x[(bits - 1) >> 5] = 1u << ((bits - 1) & 31);
  // squarings sq and start exponent s with s * 2^sq = 32 w
  uint32_t s = 32 * w, sq = 0;
  while (!(s & 1)) s >>= 1, sq++;
  for (uint32_t k = bits - 1; k < 32 * w + s; k++) {  // x = 2 x mod n
    const uint32_t top = x[w - 1] >> 31;
    for (uint32_t i = w; i-- > 1;) x[i] = (x[i] << 1) | (x[i - 1] >> 31);
    x[0] <<= 1;
    if (top || cmp_words(x, n, w) >= 0) sub_words(x, n, w);
  }
  const uint32_t np = mont_nprime(n[0]);
  std::memcpy(r2, x, sizeof(r2));  // 2^s R
  for (uint32_t k = 0; k < sq; k++) mont_mul(r2, r2, n, np, w, r2);  // 2^(32 w) R = R^2
  uint32_t base[kMaxWords];
  mont_mul(in, r2, n, np, w, base);
  int bit = 31;
  while (!((e >> bit) & 1)) bit--;
  std::memcpy(acc, base, sizeof(acc));
  for (bit--; bit >= 0; bit--) {
    mont_mul(acc, acc, n, np, w, acc);
    if ((e >> bit) & 1) mont_mul(acc, base, n, np, w, acc);
  }
  mont_mul(acc, one, n, np, w, out);
  return true;
}

// ---- SHA-256 (FIPS 180-4), byte-serial ----------------------------------------
struct Sha256 {
  uint32_t h[8];
  uint8_t buf[64];
  uint64_t len = 0;
  Sha256() {
    static const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                                   0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::memcpy(h, iv, sizeof(h));
  }
  static uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const uint8_t* p) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
        0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
        0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
        0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
        0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t w[64];
    for (int i = 0; i < 16; i++)
      w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++) {
      const uint32_t s0 = ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; i++) {
      const uint32_t t1 = hh + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
  }
  void update(const uint8_t* p, uint64_t n) {
    for (uint64_t k = 0; k < n; k++) {
      buf[len++ & 63] = p[k];
      if (!(len & 63)) block(buf);
    }
  }
  void finish(uint8_t out[32]) {
    const uint64_t bits = len * 8;
    const uint8_t pad = 0x80, zero = 0;
    update(&pad, 1);
    while ((len & 63) != 56) update(&zero, 1);
    uint8_t lb[8];
    for (int k = 0; k < 8; k++) lb[k] = (uint8_t)(bits >> (56 - 8 * k));
    update(lb, 8);
    for (int k = 0; k < 8; k++)
      for (int q = 0; q < 4; q++) out[4 * k + q] = (uint8_t)(h[k] >> (24 - 8 * q));
  }
};

// Rules 3-8 on m = s^e mod n (little-endian words, w of them): EM = I2OSP(m, emLen)
inline bool pss_check(const uint32_t* m, uint32_t w, uint32_t bits, const uint8_t* msg, uint64_t msg_len) {
  const uint32_t em_bits = bits - 1, em_len = (em_bits + 7) / 8;
  for (uint32_t k = em_len; k < 4 * w; k++)
    if ((m[k >> 2] >> (8 * (k & 3))) & 0xff) return false;  // m >= 2^(8 emLen)
  std::vector<uint8_t> em(em_len);
  for (uint32_t k = 0; k < em_len; k++) em[em_len - 1 - k] = (uint8_t)(m[k >> 2] >> (8 * (k & 3)));
  if (em[em_len - 1] != 0xbc) return false;
  const uint32_t db_len = em_len - 33;
  const uint8_t* H = em.data() + db_len;
  for (uint32_t ctr = 0; ctr * 32 < db_len; ctr++) {  // MGF1-SHA256(H, db_len)
    Sha256 s;
    const uint8_t c[4] = {(uint8_t)(ctr >> 24), (uint8_t)(ctr >> 16), (uint8_t)(ctr >> 8), (uint8_t)ctr};
    uint8_t d[32];
    s.update(H, 32);
    s.update(c, 4);
    s.finish(d);
    for (uint32_t k = 0; k < 32 && ctr * 32 + k < db_len; k++) em[ctr * 32 + k] ^= d[k];
  }
  em[0] &= (uint8_t)(0xff >> (8 * em_len - em_bits));  // cleared, never checked (BC; RFC 8017 step 6 checks)
  for (uint32_t k = 0; k + 33 < db_len; k++)
    if (em[k]) return false;
  if (em[db_len - 33] != 0x01) return false;
  uint8_t mh[32], h2[32];
  Sha256 a;
  a.update(msg, msg_len);
  a.finish(mh);
  Sha256 b;
  const uint8_t z[8] = {0};
  b.update(z, 8);
  b.update(mh, 32);
  b.update(em.data() + db_len - 32, 32);
  b.finish(h2);
  return std::memcmp(h2, H, 32) == 0;
}

// The whole lane: a CORDAHIP_STATUS_* (precedence UNSUPPORTED > BAD_KEY > EMPTY > the checks)
inline uint8_t verify(const uint8_t* key, uint64_t key_len, const uint8_t* sig, uint64_t sig_len, const uint8_t* msg,
                      uint64_t msg_len, bool do_verify) {
  PublicKey pk;
  const uint8_t ks = parse_public_key(key, key_len, pk);
  if (ks != kOk) return ks;
  if (do_verify && (sig_len == 0 || msg_len == 0)) return kEmpty;
  const uint32_t k = (pk.bits + 7) / 8, w = pk.words;
  if (sig_len > k) return kBadSig;
  uint32_t s[kMaxWords], m[kMaxWords];
  os2ip(sig, sig_len, s, w);
  if (!modexp(pk.n, pk.e, s, w, m)) return kBadSig;  // s >= n
  return pss_check(m, w, pk.bits, msg, msg_len) ? kOk : kBadSig;
}

}  // namespace rsa
}  // namespace cordahip
