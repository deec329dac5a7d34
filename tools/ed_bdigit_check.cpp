// Host check of the fixed-base digits in the Ed25519 ladder's selector stream
// (corda_amd/csrc/ed25519_sel.hpp) at the compiled width kBBits (-DED_B_BITS=16, 18
// or 20), built with ASan + UBSan by tests/test_ed_bdigits.py. For scalars e < 2^253:
//   1. the stream alone gives e back: sum_t d_t 2^(kBBits t) == e over the header's
//      kBDigitsLo + kBDigitsHi digits (so that many suffice), d_t = sel_bdigit(s, t);
//   2. every |d_t| <= 2^(kBBits - 1), and d_t == booth_digit<kBBits>(e, t);
//   3. the magnitude read from a word-major copy (stride 3, as the ladder reads its
//      LDS columns) is the same; sel_recode writes kSelWords words and no more;
//      the meta word holds nothing besides the sign bits and the count.
// Values: 0, 1, L - 1, 2^252, 2^253 - 1; chunks 2^(kBBits-1) and 2^(kBBits-1) - 1
// at even and odd positions and the other way round, which make every digit
// exactly -2^(kBBits-1) or +2^(kBBits-1); carries that ripple through every digit
// and start or end at the split between the low digits (over B) and the high
// ones (over B'); then seeded random e < L.
// Usage: ed_bdigit_check <random cases> <seed>; prints one JSON line, exit 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../corda_amd/csrc/ed25519_sel.hpp"
#include "../corda_amd/csrc/sc25519.hpp"

using namespace cordahip;
typedef unsigned __int128 u128;

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
static scalar from_u64(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  scalar s = {{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32),
               (uint32_t)d, (uint32_t)(d >> 32)}};
  return s;
}
static const scalar kL = from_u64(0x5812631a5cf5d3edull, 0x14def9dea2f79cd6ull, 0, 0x1000000000000000ull);
static bool less(const scalar& a, const scalar& b) {
  for (int i = 7; i >= 0; i--)
    if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}
// the low `bits` bits of s
static scalar truncated(scalar s, int bits) {
  for (int i = 0; i < 8; i++) {
    const int lo = 32 * i;
    if (bits <= lo) s.w[i] = 0;
    else if (bits < lo + 32) s.w[i] &= (1u << (bits - lo)) - 1;
  }
  return s;
}
static void set_bits(scalar& s, int pos, uint32_t v, int n) {  // s |= v << pos, the bits from 256 up dropped
  for (int b = 0; b < n; b++)
    if (((v >> b) & 1u) && pos + b < 256) s.w[(pos + b) >> 5] |= 1u << ((pos + b) & 31);
}
// 2^a - 2^b, a > b
static scalar pow2_diff(int a, int b) {
  scalar s = from_u64(0, 0, 0, 0);
  for (int i = b; i < a; i++) set_bits(s, i, 1, 1);
  return s;
}
// chunk i of kBBits bits = even_chunk for even i, odd_chunk for odd i, below 2^253
static scalar chunks(uint32_t even_chunk, uint32_t odd_chunk) {
  scalar s = from_u64(0, 0, 0, 0);
  for (int i = 0; kBBits * i < 253; i++) set_bits(s, kBBits * i, (i & 1) ? odd_chunk : even_chunk, kBBits);
  return truncated(s, 253);
}

// acc = acc * 2^shift + d over five u64 words of two's complement
struct acc320 {
  uint64_t w[5] = {0, 0, 0, 0, 0};
  void step(int shift, int d) {
    for (int i = 4; i > 0; i--) w[i] = (w[i] << shift) | (w[i - 1] >> (64 - shift));
    w[0] <<= shift;
    const uint64_t ext = d < 0 ? ~0ull : 0ull;
    unsigned carry = 0;
    for (int i = 0; i < 5; i++) {
      const u128 t = (u128)w[i] + (i ? ext : (uint64_t)(int64_t)d) + carry;
      w[i] = (uint64_t)t;
      carry = (unsigned)(t >> 64);
    }
  }
  bool equals(const scalar& s) const {
    for (int i = 0; i < 4; i++)
      if (w[i] != (((uint64_t)s.w[2 * i + 1] << 32) | s.w[2 * i])) return false;
    return w[4] == 0;
  }
};

static uint64_t n_min, n_max, n_zero, n_one;  // digits of exactly -2^(kBBits-1), +2^(kBBits-1), 0, +-1

static const char* check_case(const scalar& e) {
  const scalar z = from_u64(0, 0, 0, 0);
  std::vector<uint32_t> buf(kSelWords + 2, 0xdeadbeefu);
  uint32_t* s = buf.data() + 1;
  sel_recode(s, z.w, z.w, e.w, false);
  if (buf[0] != 0xdeadbeefu || buf[kSelWords + 1] != 0xdeadbeefu) return "guard word";
  uint32_t wide[3 * kSelWords];  // word-major with two neighbours, as the ladder's LDS columns
  for (int w = 0; w < kSelWords; w++) {
    wide[3 * w] = ~s[w];
    wide[3 * w + 1] = s[w];
    wide[3 * w + 2] = 0x55555555u ^ s[w];
  }
  const int half = 1 << (kBBits - 1);
  acc320 se;
  for (int t = kBDigits - 1; t >= 0; t--) {
    const int d = sel_bdigit(s, t);
    if (d > half || d < -half) return "digit out of range";
    if (d != booth_digit<kBBits>(e.w, t)) return "digit differs from booth_digit";
    if (sel_bmag(wide + 1, 3, t) != (uint32_t)(d < 0 ? -d : d)) return "strided magnitude";
    if (sel_bneg(s[kSelMeta], t) != (d < 0)) return "sign bit";
    n_min += d == -half;
    n_max += d == half;
    n_zero += d == 0;
    n_one += d == 1 || d == -1;
    se.step(kBBits, d);
  }
  if (!se.equals(e)) return "sum of the digits";
  if (sel_count(s) != 1) return "window count of zero scalars";
  if ((s[kSelMeta] & 0xffffu) >> kBDigits || s[kSelMeta] >> 24) return "meta word's spare bits";
  return nullptr;
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 100000;
  rng_state = argc > 2 ? strtoull(argv[2], 0, 10) : 1;
  static_assert(kBDigits * kBBits >= 254 && kBDigits == kBDigitsLo + kBDigitsHi, "digit counts");
  const uint32_t top = 1u << (kBBits - 1);
  const int split = kBDigitsLo * kBBits;
  std::vector<scalar> fixed = {
      from_u64(0, 0, 0, 0),
      from_u64(1, 0, 0, 0),
      from_u64(0x5812631a5cf5d3ecull, 0x14def9dea2f79cd6ull, 0, 0x1000000000000000ull),  // L - 1
      from_u64(0, 0, 0, 0x1000000000000000ull),                                          // 2^252
      from_u64(~0ull, ~0ull, ~0ull, 0x1fffffffffffffffull),                              // 2^253 - 1: one long carry
      chunks(top, top - 1),          // digits -2^(kBBits-1) at even positions, +2^(kBBits-1) at odd ones
      chunks(top - 1, top),          // the other way round (the lowest digit: 2^(kBBits-1) - 1)
      chunks(top, top),              // every digit takes a carry and passes one on
      chunks(2 * top - 1, top),
      pow2_diff(253, kBBits - 1),    // a carry from the lowest digit to the top one
      pow2_diff(253, split - 1),     // a carry that starts in the last low digit
      pow2_diff(split, 0),           // ... that ends in the first high digit
      pow2_diff(split, split - 1),   // 2^(split - 1): the last low digit is -2^(kBBits-1), the first high one +1
      pow2_diff(split + 1, split),   // 2^split: the first high digit alone
      pow2_diff(split - 1, 0),       // the low digits' largest value without a carry
  };
  uint64_t cases = 0;
  for (const scalar& e : fixed) {
    if (const char* why = check_case(e)) {
      printf("{\"fail\": \"fixed case %llu: %s\"}\n", (unsigned long long)cases, why);
      return 1;
    }
    cases++;
  }
  const uint64_t nfixed = cases, fixed_min = n_min, fixed_max = n_max;
  for (long t = 0; t < n; t++) {
    scalar e;
    do e = truncated(from_u64(rng(), rng(), rng(), rng()), 253);
    while (!less(e, kL));
    if (const char* why = check_case(e)) {
      printf("{\"fail\": \"random case %ld: %s\"}\n", t, why);
      return 1;
    }
    cases++;
  }
  printf("{\"bits\": %d, \"digits_lo\": %d, \"digits_hi\": %d, \"sel_words\": %d, \"fixed_cases\": %llu, "
         "\"random_cases\": %llu, \"fixed_min_digits\": %llu, \"fixed_max_digits\": %llu, \"zero_digits\": %llu, "
         "\"unit_digits\": %llu}\n",
         kBBits, kBDigitsLo, kBDigitsHi, kSelWords, (unsigned long long)nfixed, (unsigned long long)(cases - nfixed),
         (unsigned long long)fixed_min, (unsigned long long)fixed_max, (unsigned long long)n_zero,
         (unsigned long long)n_one);
  return 0;
}
