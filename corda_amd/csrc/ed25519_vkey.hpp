// Window geometry of Ed25519 verification against registered public keys
// (kernel K12, ed25519_vkey.hip): constants, key-id encoding, table entry
// offsets and the digit function, in one place. Usable from host and device
// (tests/test_ed_vkey_windows.py builds tools/ed_vkey_check.cpp from it).
//
// For a registered key A the kernel computes [h](-A) as 32 mixed additions, one
// per signed 8-bit digit of h = sum_j d_j 256^j, d_j in [-127, 128], from the
// key's table [d 256^j](-A), d = 1..128, j = 0..31 (affine niels entries of
// 128 bytes, the layout load_niels reads): no doublings. [S_eff]B is computed
// the same way from a table of the same shape for +B, which sits behind the
// keys' tables (slot kVkeyBaseSlot, built with the first key): the 16-bit
// fixed-base tables of the generic ladder (ed25519_ws.hpp) hold [k]B and
// [k][2^128]B for one digit position each and lean on the ladder's doublings
// for the other seven, so they cannot serve a sum without doublings. The digits are the
// bytes of h + 0x7f7f..7f minus 127 each: byte j plus the carry from below is
// v in [0, 256]; v > 128 becomes v - 256 and carries 1 into byte j + 1, which
// is what adding 0x7f to every byte does. For h < L < 2^253 byte 31 is at most
// 0x10, so digit 31 is at most 17 and no carry leaves it.
//
// A public key is public: the gathers are indexed by the lane's own digits
// (nothing here is constant-time, unlike the signer's ed25519_comb.hpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VKEY_HD __host__ __device__ inline
#else
#define VKEY_HD inline
#endif

namespace cordahip {

static constexpr int kVkeyDigits = 32;        // positions j: 256^j
static constexpr int kVkeyEntries = 128;      // |d| = 1..128 per position
static constexpr int kVkeyEntryWords = 32;    // affine niels, the entry layout of ed25519_ws.hpp
static constexpr uint32_t kVkeyTableWords = kVkeyDigits * kVkeyEntries * kVkeyEntryWords;  // 512 KiB per key

// The verification-key table of one device: kVkeySlots window tables and the
// table of B, then kVkeySlots records of 64 bytes -- the canonical Abyte SHA-512
// hashes, the key id, a live word -- then the scratch the build kernel takes
// the 32 key bytes from and leaves its decode verdict in. 65 x 512 KiB = 32.5 MiB
// of tables.
static constexpr uint32_t kVkeySlotBits = 6;
static constexpr uint32_t kVkeySlots = 1u << kVkeySlotBits;  // CORDAHIP_VKEY_MAX_KEYS
static constexpr int kVkeyRecWords = 16;
static constexpr int kVkeyRecAbyte = 0, kVkeyRecId = 8, kVkeyRecLive = 9;
static constexpr uint32_t kVkeyBaseSlot = kVkeySlots;  // the table [d 256^j]B
static constexpr uint32_t kVkeyRecBase = (kVkeySlots + 1) * kVkeyTableWords;
static constexpr uint32_t kVkeyKeyWord = kVkeyRecBase + kVkeySlots * kVkeyRecWords;  // 8 words in
static constexpr uint32_t kVkeyOkWord = kVkeyKeyWord + 8;                            // 8 words out (word 0: decoded)
static constexpr uint32_t kVkeyAllWords = kVkeyKeyWord + 16;

// A key id is slot | reuse counter << kVkeySlotBits. A slot's counter grows with
// every add (1 .. kVkeyGenMax, then 1 again), so an id that was removed never
// matches the id stored in the record of the key that took its slot; counter 0
// (a zeroed record) and the all-ones counter (0xFFFFFFFF: the id a failed add
// reports) are never issued.
static constexpr uint32_t kVkeyGenMax = (1u << (32 - kVkeySlotBits)) - 2;
static constexpr uint32_t kVkeyNoId = 0xFFFFFFFFu;
VKEY_HD constexpr uint32_t vkey_make_id(uint32_t slot, uint32_t gen) { return slot | (gen << kVkeySlotBits); }
VKEY_HD constexpr uint32_t vkey_slot(uint32_t id) { return id & (kVkeySlots - 1); }
VKEY_HD constexpr uint32_t vkey_gen(uint32_t id) { return id >> kVkeySlotBits; }
VKEY_HD constexpr uint32_t vkey_next_gen(uint32_t gen) { return gen >= kVkeyGenMax ? 1u : gen + 1; }

// word offset, within a key's table, of the entry [d 256^j](-A), d = 1..128
VKEY_HD constexpr uint32_t vkey_entry_word(int j, int d) {
  return (uint32_t)(j * kVkeyEntries + d - 1) * kVkeyEntryWords;
}

// t = h + 0x7f7f..7f (no carry out for h < 2^255); digit j is byte j of t minus 127
VKEY_HD void vkey_bias(uint32_t t[8], const uint32_t h[8]) {
  uint64_t c = 0;
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)h[i] + 0x7f7f7f7fu;
    t[i] = (uint32_t)c;
    c >>= 32;
  }
}
// digit j given the word of t that holds byte j (word j / 4)
VKEY_HD int vkey_digit(uint32_t word, int j) { return (int)((word >> (8 * (j & 3))) & 0xffu) - 127; }

// all 32 digits of the little-endian scalar h[0..8); returns the carry out of
// the biased sum (0 whenever h < 2^255)
VKEY_HD uint32_t vkey_recode(int16_t d[kVkeyDigits], const uint32_t h[8]) {
  uint32_t t[8];
  uint64_t c = 0;
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)h[i] + 0x7f7f7f7fu;
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  for (int j = 0; j < kVkeyDigits; j++) d[j] = (int16_t)vkey_digit(t[j >> 2], j);
  return (uint32_t)c;
}

// one digit the long way: byte (0..255) and the carry from the digit below
// (0 / 1) -> the signed digit in [-127, 128]; carry is updated for the digit above
VKEY_HD int vkey_step(uint32_t byte, uint32_t& carry) {
  const uint32_t v = byte + carry;  // 0..256
  carry = (v + 127u) >> 8;          // 1 iff v > 128
  return (int)v - (int)(carry << 8);
}

}  // namespace cordahip
