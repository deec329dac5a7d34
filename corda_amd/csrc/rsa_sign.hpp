// RSA_SHA256 signing with registered private keys (kernel K19, rsa_sign_keyed.hip):
// the key record, how the host fills it from the CRT components and a word-serial
// host reference of exactly the kernel's schedule, in one place. Plain C++, no HIP
// (tests/test_rsa_sign_record.py builds tools/rsa_sign_check.cpp from it).
//
// The signature of one lane is s = EM^d mod n by the Chinese remainder theorem,
//   m1 = EM^dP mod p, m2 = EM^dQ mod q, h = qInv (m1 - m2) mod p, s = m2 + q h,
// EM the EMSA-PSS encoding of the message under a caller-supplied 32-byte salt
// (RFC 8017 9.1.1; tests/golden/bc_rsa_pss.py encode_em + sign_crt), released as
// k = ceil(bits(n) / 8) big-endian bytes (I2OSP). PARITY UNPINNED like every PSS rule
// of this library: neither BouncyCastle's sources nor an RSA signature exist in the
// reference; a signature is judged by its verifiers (K8, K18, OpenSSL).
//
// Widths. The modulus runs at the verifier's width class W = class_words(bits(n)) =
// 64 / 96 / 128 words, the primes at half of it, Wp = W / 2 = 32 / 48 / 64 words; a
// key whose larger prime has more than 16 W = 32 Wp bits is declined (UNSUPPORTED).
// With Rp = 2^(32 Wp), R = 2^(32 W) and mont_x(a, b) = a b Rp^-1 mod x:
//
// Reduction of EM mod x (x = p, q). EM = lo + hi Rp has 2 Wp words and neither half
// need be below x. A CIOS product mont_x(a, b) is exact and below 2 x before its one
// conditional subtraction whenever a b < Rp x, that is for ONE operand below x and the
// other merely below Rp (the running sum stays below Rp + x < 2 Rp, one bit above the
// window, whatever the operands). r2x = Rp^2 mod x < x, so
//   u    = mont_x(hi, r2x)           = hi Rp mod x          (hi < Rp, any)
//   y    = lo + u  (< Rp + x), minus x if it carried out or is >= x: y < Rp, y = EM (mod x)
//   base = mont_x(y, r2x)            = EM Rp mod x          (y < Rp, any)
// and every later operand is below x.
// Exponentiation: fixed windows of kSignWin = 3 bits over the exponent's low
// 32 ceil(pbits / 32) bits (pbits: the longer prime's bit length), ceil of that over
// kSignWin windows from the top one down, every window kSignWin squarings and one product
// with the table entry base^digit (entry 0 is Rp mod x = mont_x(r2x, 1)): no step depends
// on a digit. (The top window may reach above those bits: the exponent is zero there.)
// Recombination: m1 stays in Montgomery form, m2 = mont_q(acc, 1) is plain and may be
// >= p (whenever q > p): t = mont_p(m2, r2p) = m2 Rp mod p (m2 < Rp, any), d = m1 - t,
// plus p when it borrowed, h = mont_p(d, qInv) (plain, < p). q h < n, so with
// qR = q R mod n the full-width mont_n(qR, h) IS q h, and s = m2 + q h < n needs no
// reduction.
// Fault check: K18's chain over s with K = R^e mod n must give EM back; else the lane
// is SIGN_FAILED and releases nothing (one faulty CRT half gives away a factor of n).
#pragma once
#include <stdint.h>

#include <cstring>

#include "rsa_vkey.hpp"

namespace cordahip {
namespace rsa {

constexpr uint32_t kHalfWords = kMaxWords / 2;  // 2048-bit primes
constexpr uint32_t kSignerMaxKeys = 64;         // live RSA signing keys of a context
// window bits of the half exponentiations: 3 ships (DESIGN.md K19 has the A/B against 4
// and 5; a build with -DCORDAHIP_RSA_SIGN_WIN=w measures another)
#ifndef CORDAHIP_RSA_SIGN_WIN
#define CORDAHIP_RSA_SIGN_WIN 3
#endif
constexpr uint32_t kSignWin = CORDAHIP_RSA_SIGN_WIN;
static_assert(kSignWin >= 1 && kSignWin <= 6, "the table has 2^kSignWin entries");
constexpr uint32_t kSignSlots = 4096;           // the signer's pool (ed25519_comb.hpp kSignKeySlots)

// One key's record, as it sits in the device's table. A zeroed record (words 0) is
// live for no lane. Everything from qR down is secret.
struct SignRecord {
  uint32_t id;     // the key id; readers compare it with the lane's
  uint32_t e;      // public exponent, odd, >= 3
  uint32_t bits;   // bit length of n
  uint32_t words;  // width class W: 64, 96 or 128
  uint32_t np;     // -n^-1 mod 2^32
  uint32_t npp;    // -p^-1 mod 2^32
  uint32_t npq;    // -q^-1 mod 2^32
  uint32_t pbits;  // bit length of the longer prime: the schedule (public: half of bits)
  uint32_t n[kMaxWords];
  uint32_t K[kMaxWords];   // R^e mod n
  uint32_t qR[kMaxWords];  // q R mod n
  uint32_t p[kHalfWords], q[kHalfWords];
  uint32_t dp[kHalfWords], dq[kHalfWords];
  uint32_t qinv[kHalfWords];  // q^-1 mod p, plain
  uint32_t r2p[kHalfWords];   // Rp^2 mod p
  uint32_t r2q[kHalfWords];   // Rp^2 mod q
};
static constexpr uint32_t kSignRecWords = 8 + 3 * kMaxWords + 7 * kHalfWords;
static constexpr uint32_t kSignRecIdWord = 0, kSignRecEWord = 1, kSignRecBitsWord = 2, kSignRecWordsWord = 3,
                          kSignRecNpWord = 4, kSignRecNppWord = 5, kSignRecNpqWord = 6, kSignRecPbitsWord = 7,
                          kSignRecNWord = 8, kSignRecKWord = kSignRecNWord + kMaxWords,
                          kSignRecQRWord = kSignRecKWord + kMaxWords, kSignRecPWord = kSignRecQRWord + kMaxWords,
                          kSignRecQWord = kSignRecPWord + kHalfWords, kSignRecDpWord = kSignRecQWord + kHalfWords,
                          kSignRecDqWord = kSignRecDpWord + kHalfWords, kSignRecQinvWord = kSignRecDqWord + kHalfWords,
                          kSignRecR2pWord = kSignRecQinvWord + kHalfWords, kSignRecR2qWord = kSignRecR2pWord + kHalfWords;
static_assert(sizeof(SignRecord) == 4 * kSignRecWords && sizeof(SignRecord) == 3360, "a record is 3,360 bytes");

// The RSA signer table of one device, in words: a slot -> record index of the pool's
// 4,096 slots (record index + 1; 0: none -- a hint only: a lane's key is live when the
// record's id is the lane's and its class the launch's), kSignerMaxKeys records, and
// the scratch of the add's consistency run (one row: key id, EM / workspace words, the
// prep status, the signature slot, its length and the status).
static constexpr uint32_t kSignTabIdxWord = 0;
static constexpr uint32_t kSignTabRecBase = kSignSlots;
static constexpr uint32_t kSignTabScratch = kSignTabRecBase + kSignerMaxKeys * kSignRecWords;
static constexpr uint32_t kSignScrIdWord = kSignTabScratch;            // 1 word (4 reserved)
static constexpr uint32_t kSignScrEmWord = kSignTabScratch + 4;        // kMaxWords words
static constexpr uint32_t kSignScrStWord = kSignScrEmWord + kMaxWords; // 1 byte (4 words reserved)
static constexpr uint32_t kSignScrSigWord = kSignScrStWord + 4;        // 4 kMaxWords bytes
static constexpr uint32_t kSignScrLenWord = kSignScrSigWord + kMaxWords;  // uint16 (2 words reserved)
static constexpr uint32_t kSignScrStatusWord = kSignScrLenWord + 2;       // 1 byte (2 words reserved)
static constexpr uint32_t kSignTabWords = kSignScrStatusWord + 2;
static constexpr uint32_t kSignTabBytes = 4 * kSignTabWords;
static_assert(kSignTabBytes == 232496 && kSignTabBytes < 512 * 1024, "the table is 227 KiB");

// The CRT components as the caller hands them over: big-endian magnitudes
struct PrivateKeyIn {
  const uint8_t *p, *q, *dp, *dq, *qinv;
  uint32_t p_len, q_len, dp_len, dq_len, qinv_len;
  uint32_t e;
};

// Zero bytes with stores the optimizer cannot drop (a memset of a local that dies is a
// dead store), and a guard that does so to a buffer on every way out of its scope.
inline void wipe_bytes(void* p, size_t n) {
  volatile unsigned char* v = static_cast<volatile unsigned char*>(p);
  while (n--) *v++ = 0;
}
struct WipeOnExit {
  void* p;
  size_t n;
  ~WipeOnExit() { wipe_bytes(p, n); }
};

inline uint32_t bit_length(const uint32_t* a, uint32_t w) {
  while (w > 0 && a[w - 1] == 0) w--;
  if (!w) return 0;
  uint32_t b = (w - 1) * 32;
  for (uint32_t v = a[w - 1]; v; v >>= 1) b++;
  return b;
}

// x = 2 x mod n (x < n), w words
inline void dbl_mod_words(uint32_t* x, const uint32_t* n, uint32_t w) {
  const uint32_t top = x[w - 1] >> 31;
  for (uint32_t i = w; i-- > 1;) x[i] = (x[i] << 1) | (x[i - 1] >> 31);
  x[0] <<= 1;
  if (top || cmp_words(x, n, w) >= 0) sub_words(x, n, w);
}

// out = 2^k mod n for k >= nbits - 1 (nbits: the bit length of n), w words
inline void pow2_mod(uint32_t* out, const uint32_t* n, uint32_t nbits, uint32_t w, uint32_t k) {
  std::memset(out, 0, 4 * (size_t)w);
  out[(nbits - 1) >> 5] = 1u << ((nbits - 1) & 31);  // < n
  for (uint32_t j = nbits - 1; j < k; j++) dbl_mod_words(out, n, w);
}

// The record of the key `k` (the caller sets rec.id). kOk: rec is filled. kBadKey: a
// zero-length component; p or q even or < 3; p = q; e even or < 3; dP >= p, dQ >= q or
// qInv >= p. kUnsupported: what the GPU path declines -- bits(p q) outside 1024..4096 or
// the larger prime above 16 W bits. Anything but kOk leaves rec zeroed. Primality is not
// checked, nor that dP, dQ and qInv belong to p, q and e: sign_consistent() below does
// the latter, on the device when a key is added.
// Custody: the parsed components (v below) are wiped on every way out; no other local
// holds a secret (n, the bit lengths and the public record are public; the Montgomery
// constants are computed in place in rec, which is the caller's to wipe).
inline uint8_t build_sign_record(const PrivateKeyIn& k, SignRecord& rec) {
  std::memset(&rec, 0, sizeof rec);
  const uint8_t* src[5] = {k.p, k.q, k.dp, k.dq, k.qinv};
  uint32_t len[5] = {k.p_len, k.q_len, k.dp_len, k.dq_len, k.qinv_len};
  for (int c = 0; c < 5; c++) {
    if (len[c] == 0) return kBadKey;
    while (len[c] && src[c][0] == 0) src[c]++, len[c]--;  // leading zeros
  }
  for (int c = 0; c < 2; c++)  // odd and >= 3
    if (len[c] == 0 || !(src[c][len[c] - 1] & 1) || (len[c] == 1 && src[c][0] < 3)) return kBadKey;
  if (len[0] == len[1] && std::memcmp(src[0], src[1], len[0]) == 0) return kBadKey;
  if (!(k.e & 1) || k.e < 3) return kBadKey;
  // a prime above 2048 bits: n above 4096 bits, or the prime above 16 W
  if (len[0] > 4 * kHalfWords || len[1] > 4 * kHalfWords) return kUnsupported;
  uint32_t v[5][kHalfWords];
  const WipeOnExit wipe_v{v, sizeof v};
  bool fits[5];
  for (int c = 0; c < 5; c++) fits[c] = os2ip(src[c], len[c], v[c], kHalfWords);
  uint32_t n[kMaxWords];
  std::memset(n, 0, sizeof n);
  for (uint32_t i = 0; i < kHalfWords; i++) {  // n = p q
    uint64_t c = 0;
    for (uint32_t j = 0; j < kHalfWords; j++) {
      const uint64_t u = (uint64_t)v[0][i] * v[1][j] + n[i + j] + c;
      n[i + j] = (uint32_t)u;
      c = u >> 32;
    }
    n[i + kHalfWords] = (uint32_t)c;
  }
  const uint32_t bits = bit_length(n, kMaxWords), W = class_words(bits);
  const uint32_t pb = bit_length(v[0], kHalfWords), qb = bit_length(v[1], kHalfWords);
  const uint32_t pbits = pb > qb ? pb : qb;
  if (!W || pbits > 16 * W) return kUnsupported;
  const uint32_t wp = W / 2;
  if (!fits[2] || !fits[3] || !fits[4] || cmp_words(v[2], v[0], kHalfWords) >= 0 ||
      cmp_words(v[3], v[1], kHalfWords) >= 0 || cmp_words(v[4], v[0], kHalfWords) >= 0)
    return kBadKey;
  PublicKey pk;
  std::memcpy(pk.n, n, sizeof n);
  pk.e = k.e;
  pk.bits = bits;
  pk.words = W;
  VkeyRecord pub;
  build_vkey_record(pk, pub);
  rec.e = k.e;
  rec.bits = bits;
  rec.words = W;
  rec.np = pub.np;
  rec.npp = mont_nprime(v[0][0]);
  rec.npq = mont_nprime(v[1][0]);
  rec.pbits = pbits;
  std::memcpy(rec.n, n, sizeof n);
  std::memcpy(rec.K, pub.K, sizeof pub.K);
  std::memcpy(rec.p, v[0], sizeof v[0]);
  std::memcpy(rec.q, v[1], sizeof v[1]);
  std::memcpy(rec.dp, v[2], sizeof v[2]);
  std::memcpy(rec.dq, v[3], sizeof v[3]);
  std::memcpy(rec.qinv, v[4], sizeof v[4]);
  pow2_mod(rec.r2p, rec.p, pb, wp, 64 * wp);
  pow2_mod(rec.r2q, rec.q, qb, wp, 64 * wp);
  std::memcpy(rec.qR, rec.q, sizeof rec.q);  // q < n; q R mod n by doubling
  for (uint32_t j = 0; j < 32 * W; j++) dbl_mod_words(rec.qR, rec.n, W);
  return kOk;
}

// the windows that cover `nwords` exponent words, and window t's digit: bits
// [t kSignWin, (t + 1) kSignWin) of the kHalfWords-word exponent, zero above it
constexpr uint32_t sign_windows(uint32_t nwords) { return (32 * nwords + kSignWin - 1) / kSignWin; }
inline uint32_t sign_digit(const uint32_t* exp, uint32_t t) {
  const uint32_t b = t * kSignWin, i = b >> 5;
  const uint64_t lo = exp[i], hi = i + 1 < kHalfWords ? exp[i + 1] : 0u;
  return (uint32_t)(((hi << 32) | lo) >> (b & 31)) & ((1u << kSignWin) - 1);
}

// The host reference of the kernel's schedule, from here to sign(): what the CPU tests
// run (tools/rsa_sign_check.cpp), not the library, which signs on the device only. Its
// own secret locals are wiped on the way out; the temporaries of rsa_key.hpp's mont_mul
// and modexp_keyed, which it calls, are not.
// acc = EM^exp mod x in Montgomery form, by the kernel's schedule (the header comment):
// em is 2 wp words, x / r2 / exp wp words, pbits the record's.
inline void half_exp(const uint32_t* em, const uint32_t* x, uint32_t npx, const uint32_t* r2, const uint32_t* exp,
                     uint32_t wp, uint32_t pbits, uint32_t* acc) {
  uint32_t one[kHalfWords], y[kHalfWords], tab[1u << kSignWin][kHalfWords];
  const WipeOnExit wipe_y{y, sizeof y}, wipe_tab{tab, sizeof tab};
  std::memset(one, 0, sizeof one);
  one[0] = 1;
  mont_mul(em + wp, r2, x, npx, wp, y);  // hi Rp mod x
  uint64_t c = 0;
  for (uint32_t i = 0; i < wp; i++) {
    const uint64_t u = (uint64_t)y[i] + em[i] + c;
    y[i] = (uint32_t)u;
    c = u >> 32;
  }
  if (c || cmp_words(y, x, wp) >= 0) sub_words(y, x, wp);  // < Rp, = EM (mod x)
  mont_mul(y, r2, x, npx, wp, tab[1]);
  mont_mul(r2, one, x, npx, wp, tab[0]);
  for (uint32_t d = 2; d < (1u << kSignWin); d++) mont_mul(tab[d - 1], tab[1], x, npx, wp, tab[d]);
  std::memcpy(acc, tab[0], 4 * (size_t)wp);
  for (uint32_t t = sign_windows((pbits + 31) / 32); t-- > 0;) {
    for (uint32_t s = 0; s < kSignWin; s++) mont_mul(acc, acc, x, npx, wp, acc);
    mont_mul(acc, tab[sign_digit(exp, t)], x, npx, wp, acc);
  }
}

// s = em^d mod n for the record's key, rec.words words each, by the kernel's schedule;
// then the fault check s^e mod n == em. false (s = 0): the check failed (also em >= n).
inline bool sign_raw(const SignRecord& rec, const uint32_t* em, uint32_t* s) {
  const uint32_t W = rec.words, wp = W / 2;
  uint32_t m1[kHalfWords], m2[kHalfWords], t[kHalfWords], h[kMaxWords], one[kHalfWords], qh[kMaxWords];
  const WipeOnExit wipe_m1{m1, sizeof m1}, wipe_m2{m2, sizeof m2}, wipe_t{t, sizeof t}, wipe_h{h, sizeof h},
      wipe_qh{qh, sizeof qh};
  std::memset(one, 0, sizeof one);
  one[0] = 1;
  half_exp(em, rec.p, rec.npp, rec.r2p, rec.dp, wp, rec.pbits, m1);  // Montgomery form
  half_exp(em, rec.q, rec.npq, rec.r2q, rec.dq, wp, rec.pbits, m2);
  mont_mul(m2, one, rec.q, rec.npq, wp, m2);      // plain, < q
  mont_mul(m2, rec.r2p, rec.p, rec.npp, wp, t);   // m2 Rp mod p (m2 < Rp, any)
  if (sub_words(m1, t, wp)) {                     // m1 - m2 mod p, Montgomery form
    uint64_t c = 0;
    for (uint32_t i = 0; i < wp; i++) {
      const uint64_t u = (uint64_t)m1[i] + rec.p[i] + c;
      m1[i] = (uint32_t)u;
      c = u >> 32;
    }
  }
  std::memset(h, 0, sizeof h);
  mont_mul(m1, rec.qinv, rec.p, rec.npp, wp, h);  // plain h < p
  mont_mul(rec.qR, h, rec.n, rec.np, W, qh);      // q h, exact
  uint64_t c = 0;
  for (uint32_t i = 0; i < W; i++) {
    const uint64_t u = (uint64_t)qh[i] + (i < wp ? m2[i] : 0u) + c;
    s[i] = (uint32_t)u;
    c = u >> 32;
  }
  uint32_t back[kMaxWords];
  VkeyRecord pub;
  std::memset(&pub, 0, sizeof pub);
  pub.e = rec.e;
  pub.words = W;
  pub.np = rec.np;
  std::memcpy(pub.n, rec.n, sizeof pub.n);
  std::memcpy(pub.K, rec.K, sizeof pub.K);
  const bool ok = !c && modexp_keyed(pub, s, back) && cmp_words(back, em, W) == 0;
  if (!ok) wipe_bytes(s, 4 * (size_t)W);  // an unconfirmed s may give away a factor of n
  return ok;
}

// The fixed EM of an add's consistency run: the bytes 0x5a below bit bits - 2 (< n)
inline void consistency_em(uint32_t bits, uint32_t W, uint32_t* em) {
  for (uint32_t i = 0; i < W; i++) {
    const uint32_t lo = 32 * i;
    em[i] = lo + 32 <= bits - 2 ? 0x5a5a5a5au : lo >= bits - 2 ? 0u : 0x5a5a5a5au & ((1u << (bits - 2 - lo)) - 1);
  }
}
// whether the record's dP, dQ and qInv sign the fixed EM to a value its public key takes back
inline bool sign_consistent(const SignRecord& rec) {
  uint32_t em[kMaxWords], s[kMaxWords];
  consistency_em(rec.bits, rec.words, em);
  return sign_raw(rec, em, s);
}

// EM = EMSA-PSS-ENCODE(msg, bits - 1) with SHA-256, MGF1-SHA-256 and the 32-byte salt,
// as W little-endian words (RFC 8017 9.1.1; bc_rsa_pss.encode_em)
inline void encode_em(const uint8_t* msg, uint64_t msg_len, const uint8_t salt[32], uint32_t bits, uint32_t W,
                      uint32_t* em) {
  const uint32_t em_bits = bits - 1, em_len = (em_bits + 7) / 8, db_len = em_len - 33;
  uint8_t mh[32], H[32], z[8] = {0};
  Sha256 a;
  a.update(msg, msg_len);
  a.finish(mh);
  Sha256 b;
  b.update(z, 8);
  b.update(mh, 32);
  b.update(salt, 32);
  b.finish(H);
  std::vector<uint8_t> e(em_len, 0);
  e[db_len - 33] = 1;
  std::memcpy(e.data() + db_len - 32, salt, 32);
  for (uint32_t ctr = 0; ctr * 32 < db_len; ctr++) {
    Sha256 s;
    const uint8_t c[4] = {(uint8_t)(ctr >> 24), (uint8_t)(ctr >> 16), (uint8_t)(ctr >> 8), (uint8_t)ctr};
    uint8_t d[32];
    s.update(H, 32);
    s.update(c, 4);
    s.finish(d);
    for (uint32_t k = 0; k < 32 && ctr * 32 + k < db_len; k++) e[ctr * 32 + k] ^= d[k];
  }
  e[0] &= (uint8_t)(0xff >> (8 * em_len - em_bits));
  std::memcpy(e.data() + db_len, H, 32);
  e[em_len - 1] = 0xbc;
  os2ip(e.data(), em_len, em, W);
}

// The whole lane on the host: sig receives k = ceil(bits / 8) big-endian bytes. false: SIGN_FAILED.
inline bool sign(const SignRecord& rec, const uint8_t* msg, uint64_t msg_len, const uint8_t salt[32], uint8_t* sig) {
  uint32_t em[kMaxWords], s[kMaxWords];
  encode_em(msg, msg_len, salt, rec.bits, rec.words, em);
  const bool ok = sign_raw(rec, em, s);
  const uint32_t k = (rec.bits + 7) / 8;
  for (uint32_t b = 0; b < k; b++) sig[k - 1 - b] = (uint8_t)(s[b >> 2] >> (8 * (b & 3)));
  return ok;
}

}  // namespace rsa
}  // namespace cordahip
