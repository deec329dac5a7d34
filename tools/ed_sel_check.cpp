// Host check of the Ed25519 ladder's selector stream (corda_amd/csrc/ed25519_sel.hpp),
// built with ASan + UBSan by tests/test_ed_sel_recode.py. For scalars (|c0|, c1, e)
// and both signs of c0 it compares what sel_recode writes with the recoding the
// ladder used to do window by window:
//   1. every window's selector with joint_select(joint_booth2(|c0|, j), joint_booth2(c1, j),
//      c0neg); the windows at or above the lane's count select the identity;
//   2. the window count with (bitlen(max(|c0|, c1)) + 2) / 2;
//   3. the kBDigits fixed-base digits (magnitude 0 .. 2^(kBBits - 1) and sign) with
//      booth_digit<kBBits>(e, t) (the header's width, ED_B_BITS; tools/ed_bdigit_check.cpp
//      covers the digits' extremes at every width);
//   4. the stream alone gives the scalars back: decoding each byte to its digit
//      pair, sum_j da_j 4^j == |c0| and sum_j dr_j 4^j == c1 over the count's
//      windows, and sum_t d_t 2^(kBBits t) == e.
// Usage: ed_sel_check <random cases> <seed>; prints one JSON line, exit 0 = pass.
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
static int bitlen(const scalar& s) {
  int n = 0;
  for (int i = 0; i < 8; i++)
    if (s.w[i]) n = 32 * i + 32 - __builtin_clz(s.w[i]);
  return n;
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

// the digit pair (i, j) of the stored entry idx: the inverse of joint_index
static void entry_digits(int idx, int& i, int& j) {
  if (idx < 2) {
    i = 0;
    j = idx + 1;
  } else {
    i = (idx - 2) / 5 + 1;
    j = (idx - 2) % 5 - 2;
  }
}

static const char* check_case(const scalar& c0abs, const scalar& c1, const scalar& e, bool c0neg) {
  // the stream sits between guard words: sel_recode writes kSelWords words and no more
  std::vector<uint32_t> buf(kSelWords + 2, 0xdeadbeefu);
  uint32_t* s = buf.data() + 1;
  sel_recode(s, c0abs.w, c1.w, e.w, c0neg);
  if (buf[0] != 0xdeadbeefu || buf[kSelWords + 1] != 0xdeadbeefu) return "guard word";
  const int bits = bitlen(c0abs) > bitlen(c1) ? bitlen(c0abs) : bitlen(c1);
  const int count = (bits + 2) / 2;
  if (sel_count(s) != count) return "window count";
  acc320 sa, sr;
  for (int j = kSelWindows - 1; j >= 0; j--) {
    const joint_sel want = joint_select(joint_booth2(c0abs.w, 1, 8, j), joint_booth2(c1.w, 1, 8, j), c0neg);
    const uint32_t got = sel_window(s, j);
    const uint32_t want_byte = (want.idx == kJointIdentity ? kSelIdentity : (uint32_t)want.idx) | (want.neg ? kSelNeg : 0u);
    if (got != want_byte) return "selector";
    if (j >= count && got != kSelIdentity) return "window above the count";
    // the digits the byte stands for
    int da = 0, dr = 0;
    if ((got & 15u) != kSelIdentity) {
      if ((int)(got & 15u) >= kJointEntries) return "entry index";
      entry_digits((int)(got & 15u), da, dr);
      if (joint_index(da, dr) != (int)(got & 15u)) return "entry_digits";
      if (got & kSelNeg) {
        da = -da;
        dr = -dr;
      }
      if (c0neg) da = -da;
    } else if (got & kSelNeg) {
      return "negated identity";
    }
    if (j < count) {
      sa.step(2, da);
      sr.step(2, dr);
    }
  }
  if (!sa.equals(c0abs) || !sr.equals(c1)) return "sum of 2-bit digits";
  acc320 se;
  for (int t = kBDigits - 1; t >= 0; t--) {
    const int want = booth_digit<kBBits>(e.w, t), got = sel_bdigit(s, t);
    if (got != want) return "fixed-base digit";
    const int mag = (int)sel_bmag(s, 1, t);
    if (mag > (1 << (kBBits - 1)) || mag != (want < 0 ? -want : want)) return "fixed-base magnitude";
    if ((((s[kSelMeta] >> t) & 1u) != 0) != (want < 0)) return "fixed-base sign";
    se.step(kBBits, got);
  }
  if (!se.equals(e)) return "sum of the fixed-base digits";
  if ((s[kSelMeta] & 0xffffu) >> kBDigits) return "sign bits past the digits";
  if ((s[kSelMeta] >> 24) != 0) return "meta word's spare bits";
  return nullptr;
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 100000;
  rng_state = argc > 2 ? strtoull(argv[2], 0, 10) : 1;
  uint64_t cases = 0;
  const uint64_t A = 0xaaaaaaaaaaaaaaaaull, F = 0x5555555555555555ull;
  // 0, 1, 2^127, 2^128 - 1, 2^128, 2^129 - 1, the alternating patterns over 128
  // and over 256 bits; around the first bit that makes sel_recode take its
  // high windows: 2^158, 2^159 - 1, 2^159; the longest: 2^255, 2^256 - 1
  const scalar half[] = {from_u64(0, 0, 0, 0),         from_u64(1, 0, 0, 0),          from_u64(0, 1ull << 63, 0, 0),
                         from_u64(~0ull, ~0ull, 0, 0), from_u64(0, 0, 1, 0),          from_u64(~0ull, ~0ull, 1, 0),
                         from_u64(A, A, 0, 0),         from_u64(F, F, 0, 0),          from_u64(A, A, A, A),
                         from_u64(F, F, F, F),         from_u64(0, 0, 1ull << 30, 0), from_u64(~0ull, ~0ull, 0x7fffffffull, 0),
                         from_u64(0, 0, 1ull << 31, 0), from_u64(0, 0, 0, 1ull << 63), from_u64(~0ull, ~0ull, ~0ull, ~0ull)};
  // e < L < 2^253: 0, 1, L - 1, 2^252, 2^253 - 1 and the patterns with the top bits set
  const scalar es[] = {from_u64(0, 0, 0, 0),
                       from_u64(1, 0, 0, 0),
                       from_u64(0x5812631a5cf5d3ecull, 0x14def9dea2f79cd6ull, 0, 0x1000000000000000ull),
                       from_u64(0, 0, 0, 0x1000000000000000ull),
                       from_u64(~0ull, ~0ull, ~0ull, 0x1fffffffffffffffull),
                       from_u64(A, A, A, A & 0x1fffffffffffffffull),
                       from_u64(F, F, F, F & 0x1fffffffffffffffull),
                       from_u64(0x8000800080008000ull, 0x8000800080008000ull, 0x8000800080008000ull, 0x1000800080008000ull),
                       from_u64(0x7fff7fff7fff7fffull, 0x7fff7fff7fff7fffull, 0x7fff7fff7fff7fffull, 0x1fff7fff7fff7fffull)};
  for (const scalar& a : half)
    for (const scalar& r : half)
      for (const scalar& e : es)
        for (int neg = 0; neg < 2; neg++) {
          if (const char* why = check_case(a, r, e, neg != 0)) {
            printf("{\"fail\": \"fixed case %llu: %s\"}\n", (unsigned long long)cases, why);
            return 1;
          }
          cases++;
        }
  const uint64_t fixed = cases;
  for (long t = 0; t < n; t++) {
    // lengths around the 128 bits the half-size scalars mostly have, now and then any length up to 256
    const int ba = (t % 7 == 0) ? (int)(rng() % 257) : 120 + (int)(rng() % 15);
    const int br = (t % 11 == 0) ? (int)(rng() % 257) : 120 + (int)(rng() % 15);
    const scalar a = truncated(from_u64(rng(), rng(), rng(), rng()), ba);
    const scalar r = truncated(from_u64(rng(), rng(), rng(), rng()), br);
    scalar e = truncated(from_u64(rng(), rng(), rng(), rng()), 253);
    if (t % 5 == 0) e.w[7] |= 0x1c000000u;  // top bits set
    if (const char* why = check_case(a, r, e, (rng() & 1) != 0)) {
      printf("{\"fail\": \"random case %ld: %s\"}\n", t, why);
      return 1;
    }
    cases++;
  }
  printf("{\"fixed_cases\": %llu, \"random_cases\": %llu}\n", (unsigned long long)fixed, (unsigned long long)(cases - fixed));
  return 0;
}
