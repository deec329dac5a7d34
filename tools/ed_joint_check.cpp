// Host check of the Ed25519 ladder's joint recoding (corda_amd/csrc/ed25519_joint.hpp),
// built with ASan + UBSan by tests/test_ed_joint_recode.py:
//   1. the 2-bit Booth digits of a scalar are in [-2, 2] and sum_j d_j 4^j is the
//      scalar, over exactly the (bitlen + 2) / 2 windows the ladder runs;
//   2. for all 25 digit pairs and both signs of c0, joint_select names the entry
//      and the negation that give da (+-P) + dr Q, with the group modelled as
//      the integers mod L (the Ed25519 group order) and the table filled in the
//      order the prep builds it.
// Usage: ed_joint_check <random cases> <seed>; prints one JSON line, exit 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../corda_amd/csrc/ed25519_joint.hpp"

using namespace cordahip;
typedef unsigned __int128 u128;

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// a scalar as the ladder holds it: 8 little-endian words, here of at most 192 bits
struct scalar {
  uint32_t w[8];
};
static scalar from_parts(uint64_t lo, uint64_t mid, uint64_t hi) {
  scalar s = {{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)mid, (uint32_t)(mid >> 32), (uint32_t)hi,
               (uint32_t)(hi >> 32), 0u, 0u}};
  return s;
}
static int bitlen(const scalar& s) {
  int n = 0;
  for (int i = 0; i < 8; i++)
    if (s.w[i]) n = 32 * i + 32 - __builtin_clz(s.w[i]);
  return n;
}

// sum_j d_j 4^j over the ladder's window count, as a 192-bit two's complement
// accumulator (three u64 words), compared with the scalar
static bool check_scalar(const scalar& s, int stride) {
  // the ladder reads its scalars from a word-major column: exercise the stride
  std::vector<uint32_t> col((size_t)8 * stride, 0xdeadbeefu);
  for (int i = 0; i < 8; i++) col[(size_t)i * stride] = s.w[i];
  const int W = (bitlen(s) + 2) / 2;
  uint64_t acc[3] = {0, 0, 0};
  for (int j = W - 1; j >= 0; j--) {
    const int d = joint_booth2(col.data(), stride, 8, j);
    if (d < -2 || d > 2) return false;
    // acc = 4 acc + d
    acc[2] = (acc[2] << 2) | (acc[1] >> 62);
    acc[1] = (acc[1] << 2) | (acc[0] >> 62);
    acc[0] <<= 2;
    const uint64_t add[3] = {(uint64_t)(int64_t)d, d < 0 ? ~0ull : 0ull, d < 0 ? ~0ull : 0ull};
    unsigned carry = 0;
    for (int i = 0; i < 3; i++) {
      const u128 t = (u128)acc[i] + add[i] + carry;
      acc[i] = (uint64_t)t;
      carry = (unsigned)(t >> 64);
    }
  }
  // every digit past the last window is zero
  for (int j = W; j < 130; j++)
    if (joint_booth2(col.data(), stride, 8, j) != 0) return false;
  for (int i = 0; i < 3; i++)
    if (acc[i] != (((uint64_t)s.w[2 * i + 1] << 32) | s.w[2 * i])) return false;
  return true;
}

// the group as Z / L, L = 2^252 + 27742317777372353535851937790883648493 the
// order of the Ed25519 base point; elements are four little-endian u64 words < L
struct zl {
  uint64_t w[4];
  bool operator==(const zl& o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
};
static const zl kL = {{0x5812631a5cf5d3edull, 0x14def9dea2f79cd6ull, 0ull, 0x1000000000000000ull}};
static bool zl_ge(const zl& a, const zl& b) {
  for (int i = 3; i >= 0; i--)
    if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
  return true;
}
static zl zl_sub_raw(const zl& a, const zl& b) {  // a >= b
  zl r;
  unsigned borrow = 0;
  for (int i = 0; i < 4; i++) {
    const u128 t = (u128)a.w[i] - b.w[i] - borrow;
    r.w[i] = (uint64_t)t;
    borrow = (unsigned)(t >> 64) & 1u;
  }
  return r;
}
static zl zl_add(const zl& a, const zl& b) {  // a, b < L < 2^253: no carry out
  zl r;
  unsigned carry = 0;
  for (int i = 0; i < 4; i++) {
    const u128 t = (u128)a.w[i] + b.w[i] + carry;
    r.w[i] = (uint64_t)t;
    carry = (unsigned)(t >> 64);
  }
  return zl_ge(r, kL) ? zl_sub_raw(r, kL) : r;
}
static zl zl_neg(const zl& a) {
  const zl zero = {{0, 0, 0, 0}};
  return a == zero ? zero : zl_sub_raw(kL, a);
}
static zl zl_small(int k, const zl& a) {  // k a, |k| <= 2
  zl r = {{0, 0, 0, 0}};
  for (int i = 0; i < (k < 0 ? -k : k); i++) r = zl_add(r, a);
  return k < 0 ? zl_neg(r) : r;
}
static zl zl_random() {
  zl r;
  do {
    for (int i = 0; i < 4; i++) r.w[i] = rng();
    r.w[3] &= 0x1fffffffffffffffull;
  } while (zl_ge(r, kL));
  return r;
}

static bool check_select(uint64_t& cases) {
  for (int rep = 0; rep < 64; rep++) {
    const zl P = zl_random(), Q = zl_random();
    // the table as the prep fills it (ed25519.hip joint_single_pass / joint_sign_pass)
    zl tab[kJointEntries];
    bool filled[kJointEntries] = {};
    auto put = [&](int i, int j, const zl& v) {
      const int idx = joint_index(i, j);
      if (idx < 0 || idx >= kJointEntries || filled[idx]) return false;
      tab[idx] = v;
      filled[idx] = true;
      return true;
    };
    bool ok = put(1, 0, P) && put(2, 0, zl_add(P, P)) && put(0, 1, Q) && put(0, 2, zl_add(Q, Q));
    for (int s = -1; s <= 1 && ok; s += 2) {
      const zl sQ = zl_small(s, Q), D = zl_add(P, sQ);
      ok = put(1, s, D) && put(1, 2 * s, zl_add(D, sQ)) && put(2, s, zl_add(D, P)) && put(2, 2 * s, zl_add(D, D));
    }
    if (!ok) return false;
    for (int i = 0; i < kJointEntries; i++)
      if (!filled[i]) return false;
    for (int c0neg = 0; c0neg < 2; c0neg++)
      for (int da = -2; da <= 2; da++)
        for (int dr = -2; dr <= 2; dr++) {
          const joint_sel sel = joint_select(da, dr, c0neg != 0);
          const zl want = zl_add(zl_small(c0neg ? -da : da, P), zl_small(dr, Q));
          if (da == 0 && dr == 0) {
            // exactly the identity, never a table entry
            if (sel.idx != kJointIdentity) return false;
          } else {
            if (sel.idx < 0 || sel.idx >= kJointEntries) return false;
            const zl got = sel.neg ? zl_neg(tab[sel.idx]) : tab[sel.idx];
            if (!(got == want)) return false;
          }
          cases++;
        }
  }
  return true;
}

int main(int argc, char** argv) {
  const long n = argc > 1 ? atol(argv[1]) : 100000;
  rng_state = argc > 2 ? strtoull(argv[2], 0, 10) : 1;
  uint64_t scalars = 0, select_cases = 0;
  const scalar fixed[] = {from_parts(0, 0, 0), from_parts(1, 0, 0), from_parts(0, 1ull << 63, 0),
                          from_parts(~0ull, ~0ull, 0), from_parts(0, 0, 1ull << 3)};  // 0, 1, 2^127, 2^128 - 1, 2^131
  for (const scalar& s : fixed) {
    if (!check_scalar(s, 1) || !check_scalar(s, 256)) {
      printf("{\"fail\": \"fixed scalar %llu\"}\n", (unsigned long long)scalars);
      return 1;
    }
    scalars++;
  }
  for (long t = 0; t < n; t++) {
    const int bits = 120 + (int)(rng() % 13);  // 120 .. 132
    uint64_t lo = rng(), mid = rng(), hi = rng();
    // exactly `bits` bits: clear above, set the top one
    if (bits <= 128) {
      hi = 0;
      mid &= ~0ull >> (128 - bits);
      mid |= 1ull << (bits - 65);
    } else {
      hi &= (1ull << (bits - 128)) - 1;
      hi |= 1ull << (bits - 129);
    }
    const scalar s = from_parts(lo, mid, hi);
    if (bitlen(s) != bits || !check_scalar(s, (t & 1) ? 256 : 1)) {
      printf("{\"fail\": \"random scalar %ld of %d bits\"}\n", t, bits);
      return 1;
    }
    scalars++;
  }
  if (!check_select(select_cases)) {
    printf("{\"fail\": \"select\"}\n");
    return 1;
  }
  printf("{\"scalars\": %llu, \"select_cases\": %llu}\n", (unsigned long long)scalars, (unsigned long long)select_cases);
  return 0;
}
