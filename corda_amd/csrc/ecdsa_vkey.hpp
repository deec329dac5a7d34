// Window geometry of ECDSA verification against registered public keys
// (kernel K13, ecdsa_vkey.hip): constants, table and record offsets, the digit
// function and the order of additions, in one place. Usable from host and
// device (tests/test_ec_vkey_windows.py builds tools/ec_vkey_check.cpp from it).
//
// For a registered key Q a lane computes P = [u1]G + [u2]Q as 64 mixed additions,
// one per signed 8-bit digit of each scalar, u = +- sum_j d_j 256^j with
// d_j in [-127, 128], from the key's table [d 256^j]Q, d = 1..128, j = 0..31, and
// from a table of the same shape for the curve's base point: no doublings.
// Entries are affine, canonical, in Montgomery form (fp29.hpp), in the 20-word
// layout ecdsa.hip's load_g reads: x[9], y[9], 2 words of padding.
//
// Digits. u < n reaches 2^256 - 1 on both curves, so Ed25519's argument (K12:
// byte 31 of h < 2^253 is small) does not hold. The scalar is first replaced by
// (u', neg) = u < 2^255 ? (u, false) : (n - u, true) -- ec_vkey_split_sign below;
// n < 2^256 gives u' < 2^255 -- and [u]X = neg ? -[u']X : [u']X. The digits of u'
// are the bytes of t = u' + 0x7f7f..7f minus 127 each (byte j plus the carry from
// below is v in [0, 256]; v > 128 becomes v - 256 and carries 1 into byte j + 1,
// which is what adding 0x7f to every byte does). u' < 2^255 keeps the top word
// of t below 2^32 (static_assert below): no carry leaves digit 31.
//
// Order of additions (fixed here so that the CPU model, the kernel and the
// tests agree on which lanes meet jmadd's exceptional branches): j from 31 down
// to 0, at each position the base point's entry and then the key's; a zero
// digit adds nothing.
//
// Key ids, slots and the reuse counter are the Ed25519 registry's
// (ed25519_vkey.hpp): one pool of kVkeySlots slots per context. A slot's record
// here is zero while the slot holds an Ed25519 key, and the other way round.
#pragma once
#include <stdint.h>

#include "ed25519_vkey.hpp"

namespace cordahip {

static constexpr int kEcVkeyEntryWords = 20;  // x[9], y[9], 2 pad: five 16-byte loads (kGEntryWords)
static constexpr uint32_t kEcVkeyTableWords = kVkeyDigits * kVkeyEntries * kEcVkeyEntryWords;  // 320 KiB per key
static_assert(kEcVkeyTableWords * 4u == 320u * 1024u, "a key's table is 320 KiB");

// The ECDSA verification-key table of one device: kVkeySlots window tables, the
// base-point tables of secp256k1 and P-256 behind them, then kVkeySlots records
// of 16 words -- scheme (2 / 3), the key id, a live word -- then the scratch the
// build kernel takes the SEC1 key bytes from (80 bytes) and leaves its decode
// verdict in. 66 x 320 KiB = 20.6 MiB of tables.
static constexpr uint32_t kEcVkeyBaseSlotK1 = kVkeySlots;      // [d 256^j]G, secp256k1 (scheme 2)
static constexpr uint32_t kEcVkeyBaseSlotR1 = kVkeySlots + 1;  // [d 256^j]G, P-256 (scheme 3)
static constexpr uint32_t kEcVkeyTables = kVkeySlots + 2;
static constexpr int kEcVkeyRecWords = 16;
static constexpr int kEcVkeyRecScheme = 0, kEcVkeyRecId = 1, kEcVkeyRecLive = 2;
static constexpr uint32_t kEcVkeyRecBase = kEcVkeyTables * kEcVkeyTableWords;
static constexpr uint32_t kEcVkeyKeyWord = kEcVkeyRecBase + kVkeySlots * kEcVkeyRecWords;  // 20 words in
static constexpr uint32_t kEcVkeyOkWord = kEcVkeyKeyWord + 20;                             // 4 words out (word 0: decoded)
static constexpr uint32_t kEcVkeyAllWords = kEcVkeyOkWord + 4;
static constexpr uint32_t kEcVkeyMaxKeyBytes = 65;  // SEC1 uncompressed

VKEY_HD constexpr uint32_t ec_vkey_base_slot(uint32_t scheme) { return scheme == 2 ? kEcVkeyBaseSlotK1 : kEcVkeyBaseSlotR1; }

// word offset, within a table, of the entry [d 256^j]X, d = 1..128
VKEY_HD constexpr uint32_t ec_vkey_entry_word(int j, int d) {
  return (uint32_t)(j * kVkeyEntries + d - 1) * kEcVkeyEntryWords;
}

// the group orders, little-endian words, for host code (the kernel passes ecdsa.hip's
// mod_m<N>(), which ecdsa.hip asserts equal to these)
static constexpr uint32_t kEcVkeyNK1[8] = {0xd0364141u, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u,
                                           0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
static constexpr uint32_t kEcVkeyNR1[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu,
                                           0xffffffffu, 0xffffffffu, 0u,          0xffffffffu};

// the largest top word of u' < 2^255, the bias word and a carry from below fit 32 bits
static_assert(0x7fffffffull + 0x7f7f7f7full + 1ull <= 0xffffffffull, "the biased sum of u' < 2^255 has no carry out");

// (u', neg): the magnitude below 2^255 and its sign, for u < n (little-endian words).
// The verify kernel calls this function and ec_vkey_bias themselves.
VKEY_HD bool ec_vkey_split_sign(uint32_t out[8], const uint32_t u[8], const uint32_t n[8]) {
  const bool neg = (u[7] >> 31) != 0;
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)n[i] - u[i] - br;
    out[i] = neg ? (uint32_t)t : u[i];
    br = (t >> 32) & 1u;
  }
  return neg;
}

// t = u' + 0x7f7f..7f; returns the carry out (0 for every u' < 2^255). Digit j of
// u' is vkey_digit(t[j / 4], j) (ed25519_vkey.hpp).
VKEY_HD uint32_t ec_vkey_bias(uint32_t t[8], const uint32_t up[8]) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)up[i] + 0x7f7f7f7fu;
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)c;
}

// all 32 digits and the sign of u < n; returns the carry out of the biased sum
VKEY_HD uint32_t ec_vkey_recode(int16_t d[kVkeyDigits], bool& neg, const uint32_t u[8], const uint32_t n[8]) {
  uint32_t up[8], t[8];
  neg = ec_vkey_split_sign(up, u, n);
  const uint32_t carry = ec_vkey_bias(t, up);
  for (int j = 0; j < kVkeyDigits; j++) d[j] = (int16_t)vkey_digit(t[j >> 2], j);
  return carry;
}

// Addition k = 0..63 of a lane: position j = 31 - k / 2, the base point's entry
// (k even) and then the key's (k odd).
VKEY_HD constexpr int ec_vkey_add_pos(int k) { return kVkeyDigits - 1 - (k >> 1); }
VKEY_HD constexpr bool ec_vkey_add_is_key(int k) { return (k & 1) != 0; }

}  // namespace cordahip
