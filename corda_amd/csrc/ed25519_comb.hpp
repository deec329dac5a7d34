// Signed 4-bit recoding of the Ed25519 signer's fixed-base scalars (kernel K11).
//
// The signer computes [r]B as 64 mixed additions from the comb table
// [d 16^j]B, d = 1..8, j = 0..63 (no doublings): r = sum_j d_j 16^j with
// d_j in [-7, 8]. Nibble j plus the carry from below is v in [0, 16]; v > 8
// becomes v - 16 and carries 1 into nibble j + 1. For r < L < 2^253 nibble 63
// is at most 1, so digit 63 is at most 2 and no carry leaves it. Every step is arithmetic on the
// value: no branch and no table lookup depends on the (secret) scalar. Usable
// from host and device (tests/test_ed_comb_recode.py builds
// tools/ed_comb_check.cpp from it).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define COMB_HD __host__ __device__ inline
#else
#define COMB_HD inline
#endif

namespace cordahip {

static constexpr int kCombDigits = 64;   // positions j: 16^j
static constexpr int kCombEntries = 8;   // |d| = 1..8 per position
static constexpr int kCombEntryWords = 32;  // affine niels, the entry layout of ed25519_ws.hpp
static constexpr int kCombTableWords = kCombDigits * kCombEntries * kCombEntryWords;  // 64 KB

// one digit: nibble (0..15) and the carry from the digit below (0 / 1) -> the
// signed digit in [-7, 8]; carry is updated for the digit above
COMB_HD int comb_step(uint32_t nibble, uint32_t& carry) {
  const uint32_t v = nibble + carry;  // 0..16
  carry = (v + 7u) >> 4;              // 1 iff v > 8
  return (int)v - (int)(carry << 4);
}

// all 64 digits of the little-endian scalar r[0..8); returns the carry out of
// digit 63 (0 whenever r < 2^253)
COMB_HD uint32_t comb_recode(int8_t d[kCombDigits], const uint32_t r[8]) {
  uint32_t carry = 0;
  for (int j = 0; j < kCombDigits; j++) d[j] = (int8_t)comb_step((r[j >> 3] >> (4 * (j & 7))) & 15u, carry);
  return carry;
}

// The signer's key table (one per device): kSignKeySlots records of 128 bytes
// -- a mod L, the 32-byte prefix, the encoded A, the key id, a live word --
// then the scratch the expansion kernel takes a seed from (and zeroes) and
// leaves the public key in. A key id is slot | generation << 12: a slot's
// generation grows with every add, so an id that was removed never matches the
// id stored in the record of the key that took its slot.
static constexpr uint32_t kSignKeySlots = 4096;
static constexpr uint32_t kSignSlotBits = 12;
static constexpr int kSignRecWords = 32;
static constexpr int kSignRecA = 0, kSignRecPrefix = 8, kSignRecPub = 16, kSignRecId = 24, kSignRecLive = 25;
static constexpr uint32_t kSignSeedWord = kSignKeySlots * kSignRecWords;  // 8 words
static constexpr uint32_t kSignPubWord = kSignSeedWord + 16;              // 8 words
static constexpr uint32_t kSignTableWords = kSignSeedWord + 32;

// index of the entry [d 16^j]B, d = 1..8
COMB_HD constexpr int comb_index(int j, int d) { return j * kCombEntries + d - 1; }

}  // namespace cordahip
