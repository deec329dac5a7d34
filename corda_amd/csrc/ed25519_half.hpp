// Which lattice vector the Ed25519 prep hands to the ladder: the end of
// half_scalars (ed25519.hip), from Euclid's state to (|c0|, sign, c1).
//
// Euclid on (8L, h), stopped at the first remainder below sqrt(8L), leaves
//   v0 = (rp, tp)  the previous remainder and its cofactor, rp >= sqrt(8L)
//   v1 = (rc, tc)  the first remainder below sqrt(8L)
// and every integer combination (c0, c1) of them has c0 == c1 h (mod 8L). The
// ladder needs c1 odd (and non-zero: an odd c1 is), and its length is
// bitlen(max(|c0|, c1)). tc odd: v1, which is short in both coordinates. tc even
// (half the lanes; tp is then odd, gcd(tp, tc) = 1): the candidates are, in
// this order,
//   v3 = v0 - q v1 (the next Euclid vector),  v1 + v3,  v1 - v3,
//   v0,  v0 + v1,  v0 - v1                                   (ED_HALF_SIX)
// all with an odd c1, and the one with the smallest max(bitlen|c0|, bitlen|c1|)
// is taken, the first of them in that order on a tie: a pure function of h. v3 is
// about 8L / rc long and v0 about 8L / |tc|, and rc |tp| + rp |tc| = 8L, so one
// of the two is short whenever the other is long; with v3's three alone about
// one lane in nine needed more than 65 ladder windows, with all six one in 23
// (tools/proto/half_scalar_windows.py: a model; the GPU figures are in DESIGN
// 9.5). Nothing bounds the length: h = L - 1 stops at v0 = (L - 1, 1),
// v1 = (8, -8), and every candidate has about 252 bits, so the ladder keeps
// its full stream.
//
// The equivalence argument above half_scalars holds for any (c0, c1) with
// c0 == c1 h (mod 8L), c1 odd: it does not care which of the candidates wins.
//
// Host and device (tests/test_ed_half_choice.py builds tools/ed_half_check.cpp
// from it): CDEV is a plain inline function for a host compiler (sc25519.hpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "sc25519.hpp"

#ifndef ED_HALF_SIX
#define ED_HALF_SIX 1  // 0: v3 and v1 +- v3 only
#endif

namespace cordahip {

// a >= b as the absence of a borrow out of a - b (branch-free: a
// short-circuit word compare becomes divergent control flow on the GPU)
CDEV bool mp8_ge(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) br = (uint32_t)(((uint64_t)a[i] - b[i] - br) >> 63);
  return br == 0;
}
CDEV void mp8_add(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a[i] + b[i];
    r[i] = (uint32_t)c;
    c >>= 32;
  }
}
CDEV void mp8_sub(uint32_t r[8], const uint32_t a[8], const uint32_t b[8]) {
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)a[i] - b[i] - br;
    r[i] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
}
CDEV void mp8_neg(uint32_t a[8]) {
  uint64_t c = 1;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)(~a[i]);
    a[i] = (uint32_t)c;
    c >>= 32;
  }
}
CDEV void mp8_copy(uint32_t d[8], const uint32_t s[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) d[i] = s[i];
}
CDEV int mp8_bits(const uint32_t a[8]) {
  int n = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) n = a[i] ? 32 * i + 32 - __builtin_clz(a[i]) : n;
  return n;
}
// bit length of |a| for a two's-complement a
CDEV int mp8_absbits(const uint32_t a[8]) {
  uint32_t t[8];
  mp8_copy(t, a);
  if (a[7] >> 31) mp8_neg(t);
  return mp8_bits(t);
}

// value of an 8-word integer as a double (relative error < 2^-49)
CDEV double mp8_f64(const uint32_t a[8]) {
  double d = (double)a[7];
#pragma unroll
  for (int i = 6; i >= 0; i--) d = fma(d, 4294967296.0, (double)a[i]);
  return d;
}
// a -= q * b  (mod 2^256), q < 2^32
CDEV void mp8_submul(uint32_t a[8], const uint32_t b[8], uint32_t q) {
  uint64_t pc = 0;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t p = (uint64_t)q * b[i] + pc;
    pc = p >> 32;
    const uint64_t d = (uint64_t)a[i] - (uint32_t)p - br;
    a[i] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
}
// o = b << k  (mod 2^256), 0 <= k < 256
CDEV void mp8_shl_dyn(uint32_t o[8], const uint32_t b[8], int k) {
  const int ws = k >> 5, bs = k & 31;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t lo = (i - ws >= 0) ? word_sel(b, i - ws) : 0u;
    const uint32_t lo2 = (i - ws - 1 >= 0) ? word_sel(b, i - ws - 1) : 0u;
    o[i] = bs ? ((lo << bs) | (lo2 >> (32 - bs))) : lo;
  }
}
CDEV uint64_t f64_bits(double d) {
  uint64_t u;
  __builtin_memcpy(&u, &d, 8);
  return u;
}
CDEV double f64_from_bits(uint64_t u) {
  double d;
  __builtin_memcpy(&d, &u, 8);
  return d;
}

// rp <- rp mod rc,  tp <- tp - (rp div rc) * tc   (mod 2^256), rc > 0.
// The quotient comes from a double-precision estimate scaled down by
// (1 - 2^-40): it never exceeds the true quotient (relative error of the
// estimate < 2^-48), so rp stays non-negative, and the loop repeats until
// rp < rc. Euclid's partial quotients are small (~1.7 bits per step), so one
// pass is the rule; a quotient >= 2^32 is taken 31 bits at a time.
CDEV void euclid_divstep(uint32_t rp[8], const uint32_t rc[8], uint32_t tp[8], const uint32_t tc[8]) {
  const double inv = 1.0 / mp8_f64(rc);
  while (mp8_ge(rp, rc)) {
    const double qd = mp8_f64(rp) * inv * (1.0 - 0x1p-40);
    if (qd < 4294967296.0) {
      uint32_t q = (uint32_t)qd;
      q = q ? q : 1u;
      mp8_submul(rp, rc, q);
      mp8_submul(tp, tc, q);
    } else {
      const int e = (int)((f64_bits(qd) >> 52) & 0x7ff) - 1023;  // qd in [2^e, 2^(e+1))
      const int k = e - 31;
      const uint32_t q = (uint32_t)(qd * f64_from_bits((uint64_t)(1023 - k) << 52));  // qd / 2^k
      uint32_t bs[8], ts[8];
      mp8_shl_dyn(bs, rc, k);
      mp8_shl_dyn(ts, tc, k);
      mp8_submul(rp, bs, q);
      mp8_submul(tp, ts, q);
    }
  }
}

// (a0, a1) <- (x0, x1) if it has an odd c1 and is strictly shorter than the best so far
CDEV void half_consider(uint32_t a0[8], uint32_t a1[8], int& best, const uint32_t x0[8], const uint32_t x1[8]) {
  const int b0 = mp8_absbits(x0), b1 = mp8_absbits(x1);
  const int b = b0 > b1 ? b0 : b1;
  // the parity guard never fires (see above); it keeps c1 odd whatever the state
  if ((x1[0] & 1u) && b < best) {
    best = b;
    mp8_copy(a0, x0);
    mp8_copy(a1, x1);
  }
}

// Euclid's state (two's-complement cofactors) -> (c0, c1): c0 == c1*h (mod 8L),
// c1 odd and positive; |c0| and its sign
CDEV void half_choose(uint32_t c0abs[8], bool& c0neg, uint32_t c1[8], const uint32_t rp[8], const uint32_t rc[8],
                      const uint32_t tp[8], const uint32_t tc[8]) {
  uint32_t a0[8], a1[8];  // chosen (c0, c1), two's complement
  mp8_copy(a0, rc);
  mp8_copy(a1, tc);
  if (!(tc[0] & 1u)) {
    int best = 1 << 30;
    uint32_t r3[8], t3[8], x0[8], x1[8];
    mp8_copy(r3, rp);
    mp8_copy(t3, tp);
    euclid_divstep(r3, rc, t3, tc);
    half_consider(a0, a1, best, r3, t3);
    mp8_add(x0, rc, r3);
    mp8_add(x1, tc, t3);
    half_consider(a0, a1, best, x0, x1);
    mp8_sub(x0, rc, r3);
    mp8_sub(x1, tc, t3);
    half_consider(a0, a1, best, x0, x1);
#if ED_HALF_SIX
    half_consider(a0, a1, best, rp, tp);
    mp8_add(x0, rp, rc);
    mp8_add(x1, tp, tc);
    half_consider(a0, a1, best, x0, x1);
    mp8_sub(x0, rp, rc);
    mp8_sub(x1, tp, tc);
    half_consider(a0, a1, best, x0, x1);
#endif
  }
  if (a1[7] >> 31) {  // make c1 positive: (c0, c1) -> (-c0, -c1)
    mp8_neg(a0);
    mp8_neg(a1);
  }
  c0neg = (a0[7] >> 31) != 0;
  if (c0neg) mp8_neg(a0);
  mp8_copy(c0abs, a0);
  mp8_copy(c1, a1);
}

}  // namespace cordahip
