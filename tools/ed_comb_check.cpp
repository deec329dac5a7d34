// Host check of the Ed25519 signer's comb recoding (corda_amd/csrc/ed25519_comb.hpp),
// built with ASan + UBSan by tests/test_ed_comb_recode.py: for every scalar r below,
// the 64 signed digits satisfy |d_j| <= 8, sum_j d_j 16^j == r (compared as 256-bit
// integers), and no carry leaves digit 63. The step-by-step form the kernel runs
// (comb_step on the low nibble of a scalar shifted right by 4 per digit) is held to
// the same digits.
//   fixed: 0, 1, L - 1, 2^252; nibbles 0..62 all 7 / 8 / 9 / f with nibble 63 = 0
//   and = 1 (the longest carry chains a scalar below 2^253 can hold; all 64 nibbles
//   7 as well); a single nibble 8 and a single nibble 9 at each position (a 9 in nibble
//   63 has no 64-digit form -- it would carry out -- and is far above 2^253: 1 there);
//   random: <count> seeded scalars reduced below L.
// Usage: ed_comb_check <random cases> <seed>; prints one JSON line, exit 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "../corda_amd/csrc/ed25519_comb.hpp"

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

// acc += d * 16^j over 9 words of two's complement (room for the intermediate sign)
static void add_digit(uint32_t acc[9], int d, int j) {
  int64_t carry = 0;
  const int word = j >> 3, sh = 4 * (j & 7);
  const int64_t v = (int64_t)d * ((int64_t)1 << sh);  // |v| < 2^32
  for (int i = word; i < 9; i++) {
    int64_t t = (int64_t)acc[i] + carry;
    if (i == word) t += v;
    acc[i] = (uint32_t)((uint64_t)t & 0xffffffffu);
    carry = t >> 32;  // arithmetic shift: floor division
  }
}

static uint64_t checked = 0, max_abs = 0, min_digit = 0, max_digit = 0;

static bool check(const scalar& s, const char* what) {
  int8_t d[kCombDigits];
  const uint32_t carry = comb_recode(d, s.w);
  if (carry) {
    fprintf(stderr, "%s: carry out of digit 63\n", what);
    return false;
  }
  uint32_t acc[9] = {0};
  for (int j = 0; j < kCombDigits; j++) {
    const int a = d[j] < 0 ? -d[j] : d[j];
    if (a > kCombEntries) {
      fprintf(stderr, "%s: digit %d is %d\n", what, j, d[j]);
      return false;
    }
    if ((uint64_t)a > max_abs) max_abs = a;
    if (d[j] < 0 && (uint64_t)-d[j] > min_digit) min_digit = -d[j];
    if (d[j] > 0 && (uint64_t)d[j] > max_digit) max_digit = d[j];
    add_digit(acc, d[j], j);
  }
  if (acc[8] != 0 || memcmp(acc, s.w, 32) != 0) {
    fprintf(stderr, "%s: digits do not sum to the scalar\n", what);
    return false;
  }
  // the kernel's form: the low nibble of a scalar shifted right by 4 per step
  uint32_t w[8], c = 0;
  memcpy(w, s.w, 32);
  for (int j = 0; j < kCombDigits; j++) {
    if (comb_step(w[0] & 15u, c) != d[j]) {
      fprintf(stderr, "%s: the shifting form differs at digit %d\n", what, j);
      return false;
    }
    for (int q = 0; q < 7; q++) w[q] = (w[q] >> 4) | (w[q + 1] << 28);
    w[7] >>= 4;
  }
  checked++;
  return c == 0;
}

static scalar nibbles(uint32_t low63, uint32_t top) {  // nibbles 0..62 = low63, nibble 63 = top
  scalar s;
  for (int i = 0; i < 8; i++) s.w[i] = low63 * 0x11111111u;
  s.w[7] = (s.w[7] & 0x0fffffffu) | (top << 28);
  return s;
}

int main(int argc, char** argv) {
  const uint64_t count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100000;
  rng_state = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
  bool ok = true;
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
  for (uint32_t v : {7u, 8u, 9u, 15u})
    for (uint32_t top : {0u, 1u}) ok &= check(nibbles(v, top), "nibbles 0..62 equal");
  ok &= check(nibbles(7, 7), "all 64 nibbles 7");
  uint64_t singles = 0;
  for (int j = 0; j < kCombDigits; j++)
    for (uint32_t v : {8u, 9u}) {
      memset(&s, 0, sizeof s);
      s.w[j >> 3] = (j == 63 && v == 9u ? 1u : v) << (4 * (j & 7));
      ok &= check(s, "single nibble");
      singles++;
    }
  uint64_t randoms = 0;
  while (randoms < count) {
    for (int i = 0; i < 8; i += 2) {
      const uint64_t x = rng();
      s.w[i] = (uint32_t)x;
      s.w[i + 1] = (uint32_t)(x >> 32);
    }
    s.w[7] &= 0x1fffffffu;  // below 2^253; then below L by rejection
    if (!below_L(s)) continue;
    ok &= check(s, "random");
    randoms++;
  }
  printf("{\"scalars\": %llu, \"singles\": %llu, \"randoms\": %llu, \"max_abs\": %llu, \"most_negative\": %llu, "
         "\"most_positive\": %llu, \"ok\": %s}\n",
         (unsigned long long)checked, (unsigned long long)singles, (unsigned long long)randoms,
         (unsigned long long)max_abs, (unsigned long long)min_digit, (unsigned long long)max_digit,
         ok ? "true" : "false");
  return ok ? 0 : 1;
}
