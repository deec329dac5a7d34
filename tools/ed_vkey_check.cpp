// Host check of the keyed Ed25519 verifier's window geometry
// (corda_amd/csrc/ed25519_vkey.hpp), built with ASan + UBSan by
// tests/test_ed_vkey_windows.py: for every scalar h below,
//   the 32 signed digits satisfy |d_j| <= 128,
//   sum_j d_j 256^j == h (compared as 256-bit integers) with no carry out of digit 31,
//   the byte-by-byte form (vkey_step) yields the same digits,
//   every nonzero digit's entry offset, plus an entry, stays inside the key's table,
// and the key-id encoding round-trips slot and counter.
//   fixed: 0, 1, L - 1, 2^252; bytes 0..30 all 0x7f / 0x80 / 0x81 with byte 31 = 0 and
//   = 0x10 (the longest carry chains a scalar below 2^253 can hold); a single byte 0x80
//   and a single byte 0x81 at each position (0x81 in byte 31 has no 32-digit form -- it
//   would carry out -- and is far above L: 1 there);
//   random: <count> seeded 512-bit values reduced below L by sc_reduce512 (sc25519.hpp).
// Usage: ed_vkey_check <random cases> <seed>; prints one JSON line, exit 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "../corda_amd/csrc/ed25519_vkey.hpp"
#include "../corda_amd/csrc/sc25519.hpp"

using namespace cordahip;

static const uint32_t kL[8] = {0x5cf5d3ed, 0x5812631a, 0xa2f79cd6, 0x14def9de, 0x0, 0x0, 0x0, 0x10000000};

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

struct scalar {
  uint32_t w[8];
};

static bool below_L(const scalar& s) {
  for (int i = 7; i >= 0; i--)
    if (s.w[i] != kL[i]) return s.w[i] < kL[i];
  return false;
}

// acc += d * 256^j over 9 words of two's complement (room for the intermediate sign)
static void add_digit(uint32_t acc[9], int d, int j) {
  int64_t carry = 0;
  const int word = j >> 2, sh = 8 * (j & 3);
  const int64_t v = (int64_t)d * ((int64_t)1 << sh);  // |v| <= 2^31
  for (int i = word; i < 9; i++) {
    int64_t t = (int64_t)acc[i] + carry;
    if (i == word) t += v;
    acc[i] = (uint32_t)((uint64_t)t & 0xffffffffu);
    carry = t >> 32;  // arithmetic shift: floor division
  }
}

static uint64_t checked = 0, max_abs = 0, min_digit = 0, max_digit = 0, zero_digits = 0;

static bool check(const scalar& s, const char* what) {
  int16_t d[kVkeyDigits];
  if (vkey_recode(d, s.w)) {
    fprintf(stderr, "%s: carry out of digit 31\n", what);
    return false;
  }
  uint32_t t[8];
  vkey_bias(t, s.w);
  uint32_t acc[9] = {0}, c = 0;
  for (int j = 0; j < kVkeyDigits; j++) {
    const int a = d[j] < 0 ? -d[j] : d[j];
    if (a > kVkeyEntries) {
      fprintf(stderr, "%s: digit %d is %d\n", what, j, d[j]);
      return false;
    }
    if ((uint64_t)a > max_abs) max_abs = a;
    if (d[j] < 0 && (uint64_t)-d[j] > min_digit) min_digit = -d[j];
    if (d[j] > 0 && (uint64_t)d[j] > max_digit) max_digit = d[j];
    zero_digits += a == 0;
    // the kernel's form: the digit from the biased scalar's word
    if (vkey_digit(t[j >> 2], j) != d[j]) {
      fprintf(stderr, "%s: the biased-word form differs at digit %d\n", what, j);
      return false;
    }
    // the long form: byte plus carry
    if (vkey_step((s.w[j >> 2] >> (8 * (j & 3))) & 0xffu, c) != d[j]) {
      fprintf(stderr, "%s: the byte-by-byte form differs at digit %d\n", what, j);
      return false;
    }
    if (a && (uint64_t)vkey_entry_word(j, a) + kVkeyEntryWords > kVkeyTableWords) {
      fprintf(stderr, "%s: digit %d = %d reads outside the table\n", what, j, d[j]);
      return false;
    }
    add_digit(acc, d[j], j);
  }
  if (c != 0 || acc[8] != 0 || memcmp(acc, s.w, 32) != 0) {
    fprintf(stderr, "%s: digits do not sum to the scalar\n", what);
    return false;
  }
  checked++;
  return true;
}

static scalar bytes31(uint32_t low31, uint32_t top) {  // bytes 0..30 = low31, byte 31 = top
  scalar s;
  for (int i = 0; i < 8; i++) s.w[i] = low31 * 0x01010101u;
  s.w[7] = (s.w[7] & 0x00ffffffu) | (top << 24);
  return s;
}

static bool check_geometry() {
  // first and last entries of a table, and the tables' place in the device allocation
  if (vkey_entry_word(0, 1) != 0) return false;
  if (vkey_entry_word(kVkeyDigits - 1, kVkeyEntries) + kVkeyEntryWords != kVkeyTableWords) return false;
  // (the keys' tables, then the base point's, then the records, then the scratch)
  if (kVkeyBaseSlot != kVkeySlots || (uint64_t)(kVkeyBaseSlot + 1) * kVkeyTableWords != kVkeyRecBase ||
      kVkeyRecBase + kVkeySlots * kVkeyRecWords != kVkeyKeyWord)
    return false;
  if (kVkeyOkWord + 8 != kVkeyAllWords || (uint64_t)kVkeyAllWords * 4 > 0xffffffffull) return false;
  // ids: slot and counter round-trip; counter 0 and the all-ones id are never issued; a
  // slot's ids differ until the counter wraps
  for (uint32_t slot = 0; slot < kVkeySlots; slot++)
    for (uint32_t gen : {1u, 2u, 77u, kVkeyGenMax - 1, kVkeyGenMax}) {
      const uint32_t id = vkey_make_id(slot, gen);
      if (vkey_slot(id) != slot || vkey_gen(id) != gen || id == kVkeyNoId) return false;
      const uint32_t nx = vkey_next_gen(gen);
      if (nx == 0 || nx > kVkeyGenMax || nx == gen || vkey_make_id(slot, nx) == kVkeyNoId) return false;
    }
  if (vkey_next_gen(0) != 1 || vkey_next_gen(kVkeyGenMax) != 1) return false;
  return vkey_slot(kVkeyNoId) == kVkeySlots - 1 && vkey_gen(kVkeyNoId) == kVkeyGenMax + 1;
}

int main(int argc, char** argv) {
  const uint64_t count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  bool ok = check_geometry();
  if (!ok) fprintf(stderr, "geometry / id encoding\n");
  scalar s;
  memset(&s, 0, sizeof s);
  ok &= check(s, "0");
  s.w[0] = 1;
  ok &= check(s, "1");
  memcpy(s.w, kL, 32);
  s.w[0] -= 1;
  ok &= check(s, "L - 1");
  memset(&s, 0, sizeof s);
  s.w[7] = 1u << 28;
  ok &= check(s, "2^252");
  for (uint32_t v : {0x7fu, 0x80u, 0x81u})
    for (uint32_t top : {0u, 0x10u}) ok &= check(bytes31(v, top), "bytes 0..30 equal");
  uint64_t singles = 0;
  for (int j = 0; j < kVkeyDigits; j++)
    for (uint32_t v : {0x80u, 0x81u}) {
      memset(&s, 0, sizeof s);
      s.w[j >> 2] = (j == 31 && v == 0x81u ? 1u : v) << (8 * (j & 3));
      ok &= check(s, "single byte");
      singles++;
    }
  uint64_t randoms = 0;
  while (randoms < count) {
    uint32_t x[16];
    for (int i = 0; i < 16; i += 2) {
      const uint64_t r = rng();
      x[i] = (uint32_t)r;
      x[i + 1] = (uint32_t)(r >> 32);
    }
    sc_reduce512(s.w, x);
    if (!below_L(s)) {
      fprintf(stderr, "sc_reduce512 left a scalar >= L\n");
      ok = false;
      break;
    }
    ok &= check(s, "random");
    randoms++;
  }
  printf("{\"scalars\": %llu, \"singles\": %llu, \"randoms\": %llu, \"max_abs\": %llu, \"most_negative\": %llu, "
         "\"most_positive\": %llu, \"zero_digits\": %llu, \"ok\": %s}\n",
         (unsigned long long)checked, (unsigned long long)singles, (unsigned long long)randoms,
         (unsigned long long)max_abs, (unsigned long long)min_digit, (unsigned long long)max_digit,
         (unsigned long long)zero_digits, ok ? "true" : "false");
  return ok ? 0 : 1;
}
