// RSA_SHA256 verification against registered public keys (kernel K18,
// rsa_vkey.hip): the key record, how the host fills it and a word-serial host
// reference of the kernel's schedule, in one place. Plain C++, no HIP
// (tests/test_rsa_vkey_record.py builds tools/rsa_vkey_check.cpp from it).
//
// A registered key keeps what rsa_modexp_kernel (K8) derives again for every
// lane: n' = -n^-1 mod 2^32 and one constant K = R^e mod n, R = 2^(32 words).
// With mont(a, b) = a b R^-1 mod n the square-and-multiply chain over the
// UNCONVERTED base, acc = in; per bit of e below its top bit acc = mont(acc, acc)
// and, the bit set, acc = mont(acc, in), yields in^e R^(1-e); the last product
// mont(acc, K) is in^e mod n. No R^2, no conversion in, none out: 16 + 1 + 1 = 18
// products for e = 65537 where K8 runs 29 (3072 bits), 3 against 14 for e = 3.
//
// Key ids, slots and the reuse counter are the verification-key registry's
// (ed25519_vkey.hpp): one pool of kVkeySlots slots per context. A slot's record
// here is zero while the slot holds a key of another family.
#pragma once
#include <stdint.h>

#include <cstring>

#include "ed25519_vkey.hpp"
#include "rsa_key.hpp"

namespace cordahip {
namespace rsa {

// One registry slot's record, as it sits in the device's table: 8 header words,
// then the modulus and K, each zero-padded to 128 words (a lane reads `words` of
// them). id 0 is never issued, so a zeroed record matches no lane.
struct VkeyRecord {
  uint32_t id;     // the key id; readers compare it with the lane's
  uint32_t e;      // public exponent, odd, >= 3
  uint32_t bits;   // bit length of the modulus
  uint32_t words;  // width class: 64, 96 or 128 (class_words)
  uint32_t np;     // -n^-1 mod 2^32
  uint32_t pad[3];
  uint32_t n[kMaxWords];
  uint32_t K[kMaxWords];  // R^e mod n, R = 2^(32 words)
};
static constexpr uint32_t kVkeyRecWords = 8 + 2 * kMaxWords;
static constexpr uint32_t kVkeyRecIdWord = 0, kVkeyRecEWord = 1, kVkeyRecBitsWord = 2, kVkeyRecWordsWord = 3,
                          kVkeyRecNpWord = 4, kVkeyRecNWord = 8, kVkeyRecKWord = 8 + kMaxWords;
static_assert(sizeof(VkeyRecord) == 4 * kVkeyRecWords && sizeof(VkeyRecord) == 1056, "a record is 1,056 bytes");
// The RSA verification-key table of one device: kVkeySlots records, 67,584 bytes (66 KiB).
static constexpr uint32_t kVkeyTableBytes = kVkeySlots * (uint32_t)sizeof(VkeyRecord);
static_assert(kVkeyTableBytes == 67584, "the table is 66 KiB");

// The record of a key parse_public_key took (pk.words != 0); the caller sets rec.id.
// R mod n by doubling 2^(bits - 1) (< n) up to 2^(32 words), K = (R mod n)^e mod n.
inline void build_vkey_record(const PublicKey& pk, VkeyRecord& rec) {
  const uint32_t w = pk.words;
  std::memset(&rec, 0, sizeof rec);
  rec.e = pk.e;
  rec.bits = pk.bits;
  rec.words = w;
  rec.np = mont_nprime(pk.n[0]);
  std::memcpy(rec.n, pk.n, 4 * (size_t)w);
  uint32_t x[kMaxWords];
  std::memset(x, 0, sizeof x);
  x[(pk.bits - 1) >> 5] = 1u << ((pk.bits - 1) & 31);
  for (uint32_t k = pk.bits - 1; k < 32 * w; k++) {  // x = 2 x mod n
    const uint32_t top = x[w - 1] >> 31;
    for (uint32_t i = w; i-- > 1;) x[i] = (x[i] << 1) | (x[i - 1] >> 31);
    x[0] <<= 1;
    if (top || cmp_words(x, pk.n, w) >= 0) sub_words(x, pk.n, w);
  }
  (void)modexp(pk.n, pk.e, x, w, rec.K);
}

// The record of the key in `der` (the SPKI BIT STRING payload): parse_public_key's
// status; anything but kOk leaves rec untouched.
inline uint8_t vkey_record_from_der(const uint8_t* der, uint64_t len, VkeyRecord& rec) {
  PublicKey pk;
  const uint8_t ks = parse_public_key(der, len, pk);
  if (ks == kOk) build_vkey_record(pk, rec);
  return ks;
}

// out = in^e mod n of the record's key over rec.words-word operands, by exactly the
// kernel's schedule (rsa_modexp_keyed_kernel): a square per bit of e below its top
// bit, a multiply per set one among them and the product with K; every operand of
// every product is < n. false (out = 0): in >= n.
inline bool modexp_keyed(const VkeyRecord& rec, const uint32_t* in, uint32_t* out) {
  const uint32_t w = rec.words;
  std::memset(out, 0, 4 * (size_t)w);
  if (cmp_words(in, rec.n, w) >= 0) return false;
  uint32_t acc[kMaxWords];
  std::memcpy(acc, in, 4 * (size_t)w);
  int bit = 31;
  while (!((rec.e >> bit) & 1)) bit--;
  for (bit--; bit >= 0; bit--) {
    mont_mul(acc, acc, rec.n, rec.np, w, acc);
    if ((rec.e >> bit) & 1) mont_mul(acc, in, rec.n, rec.np, w, acc);
  }
  mont_mul(acc, rec.K, rec.n, rec.np, w, out);
  return true;
}

}  // namespace rsa
}  // namespace cordahip
