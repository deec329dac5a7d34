// Ed25519 (EDDSA_ED25519_SHA512) batch verification for gfx950 — kernel K1,
// first half (prep) plus the fixed-base table and the corpus signer.
//
// Replaces, per lane, the reference's
//   Crypto.isValid(EDDSA_ED25519_SHA512, key, sig, clear)   Crypto.kt:534-541
//   -> i2p eddsa 0.2.0 EdDSAEngine.engineVerify (3P, semantics SURVEY App. A.1)
// with bit-exact verdicts (status byte per lane + 64-bit verdict word per
// wave via ballot). Oracle: oracle/i2p_ed25519.py, oracle/c/ed25519.c.
//
// Two kernels per batch (layout shared in ed25519_ws.hpp):
//   ed25519_prep_half_kernel (here): decode A exactly as i2p (y not range
//     checked), decode R strictly, hash the canonical re-encoding of A,
//     h = SHA-512(R||Abyte||M) mod L, S_eff from an exact emulation of
//     slide()'s carry drop, the half-size scalars (c0, c1) and e = c1 S_eff,
//     and the per-lane tables [0..8](-A), [0..8](-R) -> HBM workspace record;
//   ed25519_ladder_half_kernel (ed25519_ladder.hip): [e]B + [c0](+-A) + [c1](-R) == O.
// field products in hand-scheduled pairs (ge25519.hpp fe_mul_pair, fe25519_asm.hpp)
#ifndef FE_QUAD
#define FE_QUAD 0  // prep keeps pairs (register pressure)
#endif
#ifndef FE_USE_ASM2
#define FE_USE_ASM2 1
#endif
#include <hip/hip_runtime.h>

#include <functional>
#include <stdint.h>
#include <stdlib.h>

#include "ed25519_half.hpp"
#include "ed25519_ops.hpp"
#include "ed25519_route.hpp"
#include "ed25519_ws.hpp"
#include "sha2_device.hpp"
#include "status.hpp"

namespace cordahip {

// ---------------------------------------------------------------------------
// B table (layout: ed25519_ws.hpp), built once per context by a kernel
// (ge_base, store_niels_entry: ed25519_ops.hpp).
// tab: entries [0, kBTableEntries) = [k]B, then [k]B' with B' = [2^(kBDigitsLo kBBits)]B.
// One thread per entry: 2 (2^(kBBits-1) + 1) of them, so g and g * kBEntryWords
// stay far below 2^31 (ed25519_ws.hpp asserts the latter).
__global__ void __launch_bounds__(64) ed25519_btable_kernel(uint32_t* __restrict__ tab) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2 * kBTableEntries) return;
  const int k = g % kBTableEntries;
  ge_p3 B, P;
  ge_base(B);
  if (g >= kBTableEntries)
    for (int t = 0; t < kBDigitsLo * kBBits; t++) ge_dbl<true>(B, B);
  ge_cached bc;
  ge_to_cached(bc, B);
  ge_identity(P);
  for (int bit = kBBits - 1; bit >= 0; bit--) {
    ge_dbl<true>(P, P);
    if ((k >> bit) & 1) ge_add<true>(P, P, bc);
  }
  store_niels_entry(tab + g * kBEntryWords, P);
  if (g == 0) {
    // the joint table's shared identity entry, behind the two tables
    // (Y + X, Y - X, Z, 2dT) = (1, 1, 1, 0)
    ge_cached id;
    fe_set(id.YpX, 1);
    fe_set(id.YmX, 1);
    fe_set(id.Z, 1);
    fe_set(id.T2d, 0);
    store_cached(tab + kBIdentityWord, id);
  }
}

// ---------------------------------------------------------------------------
// Half-size scalars. With R decoded strictly,
//   encode([S]B - [h]A) == R_bytes  <=>  P := [S]B - [h]A - R == O.
// For any (c0, c1) with c0 == c1*h (mod 8L) and c1 odd, c1 != 0 (mod L):
//   [c1]P == [c1*S mod L]B - [c0]A - [c1]R,   and   [c1]P == O <=> P == O
// (A, R may carry torsion: every point's order divides 8L, so the mod-8L
// congruence makes [c0]A == [c1 h]A exact; c1 odd kills no 2-power torsion;
// c1 != 0 mod L keeps the prime-order part). Extended Euclid on (8L, h),
// stopped below sqrt(8L), gives |c0|, |c1| ~ 2^128: the ladder needs ~128
// doublings instead of ~252 (idea: T. Pornin, ePrint 2020/454). The
// equivalence is checked on the golden catalogue in tools/proto/half_scalar.py.
// Which lattice vector is taken (ed25519_half.hpp half_choose: the first short
// remainder when its cofactor is odd, else the shortest of six neighbours with
// an odd c1, the previous Euclid vector among them) does not enter the
// argument: it holds for every (c0, c1) with c0 == c1*h (mod 8L) and c1 odd.
// The multiprecision helpers and the exact division step are in that header.

// floor(a / 2^s) as a double, exact for a < 2^(s+53)
CDEV double mp8_top(const uint32_t a[8], int s) {
  const int w = s >> 5, b = s & 31;
  const uint64_t lo = ((uint64_t)word_sel(a, w + 1) << 32) | word_sel(a, w);
  const uint64_t hi = word_sel(a, w + 2);
  return (double)((lo >> b) | (b ? hi << (64 - b) : 0ull));
}
// o = a*x + b*y (mod 2^256) for |a|, |b| < 2^31 of opposite signs (or one of
// them zero), as |a|x - |b|y, negated when the positive factor is b
CDEV void mp8_lincomb(uint32_t o[8], const uint32_t x[8], int a, const uint32_t y[8], int b) {
  const uint32_t ua = (uint32_t)(a < 0 ? -a : a), ub = (uint32_t)(b < 0 ? -b : b);
  uint64_t pc = 0, qc = 0;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t p = (uint64_t)ua * x[i] + pc;
    pc = p >> 32;
    const uint64_t q = (uint64_t)ub * y[i] + qc;
    qc = q >> 32;
    const uint64_t d = (uint64_t)(uint32_t)p - (uint32_t)q - br;
    o[i] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
  if (b > 0 || (b == 0 && a < 0)) mp8_neg(o);
}

// (c0, c1): c0 == c1*h (mod 8L), c1 odd and positive; returns |c0| and its sign
CDEV void half_scalars(uint32_t c0abs[8], bool& c0neg, uint32_t c1[8], const uint32_t h[8]) {
  const uint32_t kM[8] = {0xe7ae9f68u, 0xc09318d2u, 0x17bce6b2u, 0xa6f7cef5u, 0u, 0u, 0u, 0x80000000u};  // 8L
  const uint32_t kS[8] = {0x754abea0u, 0x597d89b3u, 0xf9de6484u, 0xb504f333u, 0u, 0u, 0u, 0u};        // isqrt(8L)+1
  uint32_t rp[8], rc[8], tp[8], tc[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    rp[i] = kM[i];
    rc[i] = h[i];
    tp[i] = 0;
    tc[i] = i == 0;
  }
  // Euclid on (8L, h) until the first remainder below sqrt(8L), run as Lehmer
  // rounds (Knuth TAOCP 4.5.2, Algorithm L): Euclid on the 52-bit leading
  // parts of rp, rc (exact in doubles) while both bracketing quotients agree,
  // so every quotient is Euclid's own, then the round's 2x2 cofactor matrix
  // is applied to the 256-bit remainders and cofactors once. A step is taken
  // only while the remainder it produces provably stays >= sqrt(8L) (its
  // true value is within max(|C|,|D|) units of the leading part), so one
  // exact step below finishes. ~6 rounds of ~12 double-precision steps replace
  // ~73 multiprecision steps; the state handed over is Euclid's exactly
  // (tools/proto/lehmer.py checks that on 5e4 random h).
  for (;;) {
    const int s = max(mp8_bitlen(rp) - 52, 0);
    double uh = mp8_top(rp, s), vh = mp8_top(rc, s);
    const double th = mp8_top(kS, s) + 1.0;
    double A = 1.0, B = 0.0, C = 0.0, D = 1.0;
    int n = 0;
    for (;;) {
      const double d1 = vh + C, d2 = vh + D;
      if (!(d1 > 0.0 && d2 > 0.0)) break;
      const double n1 = uh + A;
      double q = floor(n1 / d1);
      const double r1 = fma(-q, d1, n1);  // exact: |r1| < 2^53
      q = r1 < 0.0 ? q - 1.0 : (r1 >= d1 ? q + 1.0 : q);
      const double r2 = fma(-q, d2, uh + B);
      if (!(r2 >= 0.0 && r2 < d2)) break;  // the other bracket's quotient differs
      const double nC = fma(-q, C, A), nD = fma(-q, D, B), nv = fma(-q, vh, uh);
      const double mc = fmax(fabs(nC), fabs(nD));
      if (nv - mc < th || mc >= 0x1p30) break;
      A = C;
      B = D;
      C = nC;
      D = nD;
      uh = vh;
      vh = nv;
      n++;
    }
    if (n == 0) break;
    const int a = (int)A, b = (int)B, c = (int)C, d = (int)D;
    uint32_t x[8], y[8];
    mp8_lincomb(x, rp, a, rc, b);
    mp8_lincomb(y, rp, c, rc, d);
    mp8_copy(rp, x);
    mp8_copy(rc, y);
    mp8_lincomb(x, tp, a, tc, b);
    mp8_lincomb(y, tp, c, tc, d);
    mp8_copy(tp, x);
    mp8_copy(tc, y);
  }
  // the remaining exact step(s): (rc, tc) <- the first remainder below
  // sqrt(8L) and its cofactor, (rp, tp) <- the previous one
  while (mp8_ge(rc, kS)) {
    euclid_divstep(rp, rc, tp, tc);  // rp <- rp mod rc
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t a = rp[i], b = tp[i];
      rp[i] = rc[i];
      rc[i] = a;
      tp[i] = tc[i];
      tc[i] = b;
    }
  }
  half_choose(c0abs, c0neg, c1, rp, rc, tp, tc);  // ed25519_half.hpp
}

// Strict R decode: the reference never decodes R, it compares encode(R')
// with the 32 bytes; those equal only when the bytes are the canonical
// encoding of a curve point: y < p, on the curve, not (x == 0 with bit 255).
// the extra conditions of a strict decode, given R = ge_frombytes_i2p(w) succeeded
CDEV bool ge_strict_ok(const ge_p3& R, const uint32_t w[8]) {
  uint32_t all_ones = (w[7] & 0x7fffffffu) == 0x7fffffffu;
#pragma unroll
  for (int i = 1; i < 7; i++) all_ones &= (w[i] == 0xffffffffu);
  if (all_ones && w[0] >= 0xffffffedu) return false;  // y >= p
  return !((w[7] >> 31) && fe_iszero(R.X));
}

// an affine point (Z = 1) as X, Y, T (30 words, 16-B aligned slot of 40)
CDEV void store_point(uint32_t* __restrict__ o, const ge_p3& p) {
  uint4* o4 = reinterpret_cast<uint4*>(o);
  uint32_t w[32];
#pragma unroll
  for (int i = 0; i < 10; i++) {
    w[i] = p.X.v[i];
    w[10 + i] = p.Y.v[i];
    w[20 + i] = p.T.v[i];
  }
  w[30] = w[31] = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) o4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
}
CDEV void load_point(ge_p3& p, const uint32_t* __restrict__ o) {
  const uint4* o4 = reinterpret_cast<const uint4*>(o);
  uint32_t w[32];
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const uint4 v = o4[q];
    w[4 * q] = v.x;
    w[4 * q + 1] = v.y;
    w[4 * q + 2] = v.z;
    w[4 * q + 3] = v.w;
  }
#pragma unroll
  for (int i = 0; i < 10; i++) {
    p.X.v[i] = w[i];
    p.Y.v[i] = w[10 + i];
    p.T.v[i] = w[20 + i];
  }
  fe_set(p.Z, 1);
}

// The joint table i P + j Q (P = -A, Q = -R affine; ed25519_joint.hpp) is built
// from doublings and mixed additions only, in two loops of two passes each (one
// copy of each body in the I-cache), which meet through the parked points:
//   single pass (base = P, then Q): [1]base, whose cached form with Z = 1 is
//     also its niels form, and [2]base;
//   sign pass (s = -1, then +1): D = P + sQ, 2D = 2P + 2sQ, D + sQ = P + 2sQ,
//     D + P = 2P + sQ.
// 4 doublings, 6 mixed additions, 2 + 10 products by 2d: 16 S + 70 M per lane.
// Between the passes P and Q are parked. ED_PREP_LDS: in LDS, word-major, one
// column of kPqWords per thread (256 threads: 70 KB, two blocks per CU), so no
// pass waits for a store of its own wave to come back from memory:
//   P as X, Y, T and, once its single pass has the product, 2dT: (1, 0) as
//     niels is (Y + X, Y - X, 2dT), two additions away;
//   Q as X, Y, T until its single pass has read it, then as the niels form of
//     (0, 1) in the same words (nothing later needs Q itself).
// Without it: as (X, Y, T) in the record's slots of 2P + 2Q and 2P - 2Q (Q's
// slot is free once the single passes are done, P's is written last), the
// niels forms read back from the entries (1, 0) and (0, 1).
#ifndef ED_PREP_LDS
#define ED_PREP_LDS 1
#endif
#if !ED_PREP_LDS
static constexpr int kParkP = joint_index(2, 2), kParkQ = joint_index(2, -2);
#endif
static constexpr int kPqT2d = 30, kPqQ = 40, kPqWords = 70;  // P: X Y T 2dT at 0 10 20 30; Q: three fe at 40 50 60

CDEV uint32_t* joint_slot(uint32_t* rec, int idx) { return rec + kWhTab + idx * kWhEntryWords; }

CDEV void pq_store(uint32_t* col, int at, const fe& f) {
#pragma unroll
  for (int i = 0; i < 10; i++) col[(at + i) * 256] = f.v[i];
}
CDEV void pq_load(fe& f, const uint32_t* col, int at) {
#pragma unroll
  for (int i = 0; i < 10; i++) f.v[i] = col[(at + i) * 256];
}

// an entry with Z = 1 read back as the niels form of its point
CDEV void load_cached_niels(ge_niels& n, const uint32_t* __restrict__ p) {
  ge_cached c;
  load_cached(c, p);
  n.ypx = c.YpX;
  n.ymx = c.YmX;
  n.xy2d = c.T2d;
}

// the affine point parked by the decode phase: which = 0 is P, 1 is Q
CDEV void park_point(uint32_t* __restrict__ rec, uint32_t* col, int which, const ge_p3& p) {
#if ED_PREP_LDS
  pq_store(col, which * kPqQ, p.X);
  pq_store(col, which * kPqQ + 10, p.Y);
  pq_store(col, which * kPqQ + 20, p.T);
#else
  store_point(joint_slot(rec, which ? kParkQ : kParkP), p);
#endif
}
CDEV void load_parked(ge_p3& p, uint32_t* __restrict__ rec, const uint32_t* col, int which) {
#if ED_PREP_LDS
  pq_load(p.X, col, which * kPqQ);
  pq_load(p.Y, col, which * kPqQ + 10);
  pq_load(p.T, col, which * kPqQ + 20);
  fe_set(p.Z, 1);
#else
  load_point(p, joint_slot(rec, which ? kParkQ : kParkP));
#endif
}
// a single pass has the cached form c (Z = 1) of its point: keep what the sign
// passes need of it
CDEV void park_niels(uint32_t* col, int pass, const ge_cached& c) {
#if ED_PREP_LDS
  if (pass) {
    pq_store(col, kPqQ, c.YpX);
    pq_store(col, kPqQ + 10, c.YmX);
    pq_store(col, kPqQ + 20, c.T2d);
  } else {
    pq_store(col, kPqT2d, c.T2d);
  }
#endif
}
// the niels form of P (which = 0) or Q
CDEV void load_parked_niels(ge_niels& n, uint32_t* __restrict__ rec, const uint32_t* col, int which) {
#if ED_PREP_LDS
  if (which) {
    pq_load(n.ypx, col, kPqQ);
    pq_load(n.ymx, col, kPqQ + 10);
    pq_load(n.xy2d, col, kPqQ + 20);
  } else {
    fe x, y;
    pq_load(x, col, 0);
    pq_load(y, col, 10);
    fe_add(n.ypx, y, x);  // as ge_to_cached
    fe_sub(n.ymx, y, x);
    pq_load(n.xy2d, col, kPqT2d);
  }
#else
  load_cached_niels(n, joint_slot(rec, which ? joint_index(0, 1) : joint_index(1, 0)));
#endif
}

// pass 0: [1]P, [2]P; pass 1: [1]Q, [2]Q
CDEV void joint_single_pass(uint32_t* __restrict__ rec, uint32_t* col, int pass) {
  ge_p3 B, D;
  load_parked(B, rec, col, pass);
  ge_cached c;
  ge_to_cached(c, B);
  park_niels(col, pass, c);
  store_cached(joint_slot(rec, pass ? joint_index(0, 1) : joint_index(1, 0)), c);
  ge_dbl<true>(D, B);
  ge_to_cached(c, D);
  store_cached(joint_slot(rec, pass ? joint_index(0, 2) : joint_index(2, 0)), c);
}

// the four entries that mix P and Q with relative sign s (s = -1 first: without
// ED_PREP_LDS the s = +1 pass overwrites P's parking slot with its last store)
CDEV void joint_sign_pass(uint32_t* __restrict__ rec, uint32_t* col, int s) {
  ge_p3 D, E;
  ge_niels nq, np;
  ge_cached c;
  load_parked(D, rec, col, 0);
  load_parked_niels(nq, rec, col, 1);
  niels_cneg(nq, s < 0);
  ge_madd<true>(D, D, nq);  // P + sQ
  ge_to_cached(c, D);
  store_cached(joint_slot(rec, joint_index(1, s)), c);
  ge_madd<true>(E, D, nq);  // P + 2sQ
  ge_to_cached(c, E);
  store_cached(joint_slot(rec, joint_index(1, 2 * s)), c);
#if ED_PREP_LDS
  PHASE_BARRIER();  // nothing orders the LDS reads of np behind the stores above: keep them here
#endif
  load_parked_niels(np, rec, col, 0);
  ge_madd<true>(E, D, np);  // 2P + sQ
  ge_to_cached(c, E);
  store_cached(joint_slot(rec, joint_index(2, s)), c);
  ge_dbl<true>(E, D);       // 2P + 2sQ
  ge_to_cached(c, E);
  store_cached(joint_slot(rec, joint_index(2, 2 * s)), c);
}

// ---------------------------------------------------------------------------
// Prep of the half-size-scalar verification: the ladder (ed25519_ladder.hip)
// decides [e]B + [c0](+-A) + [c1](-R) == O with ~128-bit c0, c1 (half_scalars):
// ~132 doublings instead of 252 and no final inversion (P == O is X == 0, Y == Z).
// Record layout: ed25519_ws.hpp (kWh*).

// Phases, each finished (and its table written to the workspace) before the
// next starts: decode A, strict decode R | joint table i(-A) + j(-R) |
// SHA-512, h, S_eff, lattice reduction, e = c1 S_eff mod L. Lanes whose
// status is already decided run the phases on the identity / zero scalars.
#ifndef ED_PREP_WAVES
#define ED_PREP_WAVES 2
#endif
// Phase 1 of the prep (no message) is prep_decode_phase, then prep_table_phase:
// decode A and R, the pre-engine statuses | the joint table i(-A) + j(-R).
// Returns the lane's status (kStatusPending: verify); abyte =
// EdDSAPublicKey.Abyte, Rw = R's bytes, both for the SHA-512 of phase 2. It
// leaves P = -A and Q = -R parked (ED_PREP_LDS) for the table phase.
CDEV uint8_t prep_decode_phase(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ sigs, uint64_t i,
                               uint32_t msg_len, const uint8_t* __restrict__ pre_status, uint32_t empty_is_error,
                               uint32_t* __restrict__ rec, uint32_t* col, uint32_t abyte[8], uint32_t Rw[8]) {
  uint8_t st = kStatusPending;
  load8(Rw, reinterpret_cast<const uint32_t*>(sigs + i * 64));
  {
    // A (i2p decode: y not range checked) and R (strict decode: encode(R') ==
    // Rw only if Rw is a canonical point encoding) decompressed together: the
    // two square-root exponentiations run as interleaved chains
    uint32_t wa[8];
    load8(wa, reinterpret_cast<const uint32_t*>(keys + i * 32));
    ge_p3 A, R;
    bool okA, okR;
    ge_frombytes_i2p_pair(A, okA, wa, R, okR, Rw);
    if (!okA) st = kStatusBadKey;  // key decode precedes doVerify (Kryo.kt:389-392)
    else if (pre_status && pre_status[i] != kStatusOk) st = pre_status[i];
    else if (msg_len == 0 && empty_is_error) st = kStatusEmpty;  // doVerify: Crypto.kt:476 (isValid hashes it)
    fe_tobytes(abyte, A.Y);  // EdDSAPublicKey.Abyte = A.toByteArray(): canonical
    abyte[7] |= fe_isnegative(A.X) << 31;
    if (st == kStatusPending && !(okR && ge_strict_ok(R, Rw))) st = kStatusBadSig;  // no canonical point encodes to Rw
    if (st != kStatusPending) {
      ge_identity(A);
      ge_identity(R);
    }
    // P = -A, Q = -R parked (Z = 1: X, Y, T), so the table loops below hold
    // one point at a time
    fe_neg(A.X, A.X);
    fe_neg(A.T, A.T);
    fe_neg(R.X, R.X);
    fe_neg(R.T, R.T);
    park_point(rec, col, 0, A);
    park_point(rec, col, 1, R);
  }
  return st;
}

CDEV void prep_table_phase(uint32_t* __restrict__ rec, uint32_t* col) {
  // the joint table i P + j Q: one loop body per kind of pass keeps a single
  // copy of its code in the I-cache
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
    joint_single_pass(rec, col, pass);
    PHASE_BARRIER();
  }
#pragma unroll 1
  for (int s = -1; s <= 1; s += 2) {
    joint_sign_pass(rec, col, s);
    PHASE_BARRIER();
  }
}

CDEV uint8_t prep_keys_phase(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ sigs, uint64_t i,
                             uint32_t msg_len, const uint8_t* __restrict__ pre_status, uint32_t empty_is_error,
                             uint32_t* __restrict__ rec, uint32_t* col, uint32_t abyte[8], uint32_t Rw[8]) {
  const uint8_t st = prep_decode_phase(keys, sigs, i, msg_len, pre_status, empty_is_error, rec, col, abyte, Rw);
  PHASE_BARRIER();
  prep_table_phase(rec, col);
  return st;
}

// Phase 2 (the message): SHA-512(R || A || M), h, S_eff, the lattice reduction,
// e = c1 S_eff mod L -> the record's scalars (zero for decided lanes).
CDEV void prep_msg_phase(const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ msgs, uint32_t msg_len,
                         uint64_t i, uint8_t st, const uint32_t abyte[8], const uint32_t Rw[8],
                         uint32_t* __restrict__ rec) {
  uint32_t ka[8], kr[8], e[8];
  bool c0neg = false;
  if (st == kStatusPending) {
    uint32_t S[8], hd[16], h[8], se[8], zero[8];
    load8(S, reinterpret_cast<const uint32_t*>(sigs + i * 64 + 32));
    sha512_segments(hd, Rw, abyte, true, msgs + i * (uint64_t)msg_len, msg_len);
    sc_reduce512(h, hd);
    sc_effective_S(se, S, slide_drops_carry(S));
    half_scalars(ka, c0neg, kr, h);
#pragma unroll
    for (int q = 0; q < 8; q++) zero[q] = 0;
    sc_muladd(e, kr, se, zero);  // e = c1 S_eff mod L
  } else {
#pragma unroll
    for (int q = 0; q < 8; q++) ka[q] = kr[q] = e[q] = 0;
  }
#if ED_SEL_STREAM
  // what the ladder consumes (ed25519_sel.hpp): window selectors, B digits, window count
  uint32_t sel[32];
  sel_recode(sel, ka, kr, e, c0neg);
#pragma unroll
  for (int q = kSelWords; q < 32; q++) sel[q] = 0;
  uint4* o4 = reinterpret_cast<uint4*>(rec + kWhSel);
#pragma unroll
  for (int q = 0; q < 8; q++) o4[q] = make_uint4(sel[4 * q], sel[4 * q + 1], sel[4 * q + 2], sel[4 * q + 3]);
#else
  store8(rec + kWhKa, ka);
  store8(rec + kWhKr, kr);
  store8(rec + kWhE, e);
  reinterpret_cast<uint4*>(rec + kWhFlags)[0] = make_uint4(c0neg ? 1u : 0u, 0u, 0u, 0u);
#endif
}

// this thread's column of the parking area (ED_PREP_LDS)
#if ED_PREP_LDS
#define PREP_PARK_COLUMN(col)                  \
  __shared__ uint32_t pq_lds[kPqWords][256]; \
  uint32_t* col = &pq_lds[0][threadIdx.x]
#else
#define PREP_PARK_COLUMN(col) uint32_t* col = nullptr
#endif

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ED_PREP_WAVES))) ed25519_prep_half_kernel(
    const uint8_t* __restrict__ keys, const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ msgs,
    uint32_t msg_len, uint64_t base, uint64_t m, const uint8_t* __restrict__ pre_status,
    uint8_t* __restrict__ status, uint32_t* __restrict__ ws, uint32_t empty_is_error) {
  const uint64_t li = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= m) return;
  const uint64_t i = base + li;
  uint32_t* rec = ws + li * kWhLaneWords;
  uint32_t abyte[8], Rw[8];
  PREP_PARK_COLUMN(col);
  const uint8_t st = prep_keys_phase(keys, sigs, i, msg_len, pre_status, empty_is_error, rec, col, abyte, Rw);
  prep_msg_phase(sigs, msgs, msg_len, i, st, abyte, Rw, rec);
  status[i] = st;
}

// The fused prep of a routed batch (K14, ed25519_route.hpp): workspace record li
// belongs to lane generic[base + li]; the chunk holds route_chunk_lanes(generic
// count, base, m) records, the count read from the scratch header.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ED_PREP_WAVES)))
ed25519_prep_half_idx_kernel(const uint8_t* __restrict__ keys, const uint8_t* __restrict__ sigs,
                             const uint8_t* __restrict__ msgs, uint32_t msg_len, uint64_t base, uint64_t m,
                             const uint8_t* __restrict__ pre_status, uint8_t* __restrict__ status,
                             uint32_t* __restrict__ ws, uint32_t empty_is_error, const uint32_t* __restrict__ scratch,
                             uint64_t lanes) {
  const uint64_t li = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= route_chunk_lanes(scratch[kRouteCntGeneric], base, m)) return;
  const uint64_t i = scratch[route_off_generic(lanes) + base + li];
  uint32_t* rec = ws + li * kWhLaneWords;
  uint32_t abyte[8], Rw[8];
  PREP_PARK_COLUMN(col);
  const uint8_t st = prep_keys_phase(keys, sigs, i, msg_len, pre_status, empty_is_error, rec, col, abyte, Rw);
  prep_msg_phase(sigs, msgs, msg_len, i, st, abyte, Rw, rec);
  status[i] = st;
}

// The same prep in two launches, for batches whose messages arrive after their
// keys and signatures (the signed-tx chunks: each message is its transaction's
// id, gathered on the device once the id slice is done): phase 1 needs no
// message and runs while the ids are computed; it leaves the lane's status in
// `status` and Abyte in the record's scalar words, which phase 2 overwrites.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ED_PREP_WAVES))) ed25519_prep_keys_kernel(
    const uint8_t* __restrict__ keys, const uint8_t* __restrict__ sigs, uint32_t msg_len, uint64_t base, uint64_t m,
    const uint8_t* __restrict__ pre_status, uint8_t* __restrict__ status, uint32_t* __restrict__ ws,
    uint32_t empty_is_error) {
  const uint64_t li = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= m) return;
  const uint64_t i = base + li;
  uint32_t* rec = ws + li * kWhLaneWords;
  uint32_t abyte[8], Rw[8];
  PREP_PARK_COLUMN(col);
  status[i] = prep_keys_phase(keys, sigs, i, msg_len, pre_status, empty_is_error, rec, col, abyte, Rw);
  store8(rec + kWhKa, abyte);
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ED_PREP_WAVES))) ed25519_prep_msg_kernel(const uint8_t* __restrict__ sigs,
                                                               const uint8_t* __restrict__ msgs, uint32_t msg_len,
                                                               uint64_t base, uint64_t m,
                                                               const uint8_t* __restrict__ status,
                                                               uint32_t* __restrict__ ws) {
  const uint64_t li = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (li >= m) return;
  const uint64_t i = base + li;
  uint32_t* rec = ws + li * kWhLaneWords;
  uint32_t abyte[8], Rw[8];
  load8(abyte, rec + kWhKa);
  load8(Rw, reinterpret_cast<const uint32_t*>(sigs + i * 64));
  prep_msg_phase(sigs, msgs, msg_len, i, status[i], abyte, Rw, rec);
}

// ---------------------------------------------------------------------------
// RFC 8032 keygen + sign (Crypto.doSign / deriveKeyPairFromEntropy for
// Ed25519): the GPU corpus generator for bench.py and the C5 stream.
CDEV void fixed_base_mult(ge_p3& P, const uint32_t k[8], const uint32_t* __restrict__ btab) {
  ge_identity(P);
  for (int j = 31; j >= 0; j--) {
    if (j != 31) {
#pragma unroll
      for (int t = 0; t < 7; t++) ge_dbl<false>(P, P);
      ge_dbl<true>(P, P);
    }
    const int d = booth_digit<8>(k, j);
    ge_niels nb;
    load_niels(nb, btab, d < 0 ? -d : d);
    niels_cneg(nb, d < 0);
    ge_madd<true>(P, P, nb);
  }
}

__global__ void __launch_bounds__(256) ed25519_sign_kernel(const uint8_t* __restrict__ seeds,
                                                          const uint8_t* __restrict__ msgs, uint32_t msg_len,
                                                          uint64_t n, const uint32_t* __restrict__ btab,
                                                          uint8_t* __restrict__ pubs, uint8_t* __restrict__ sigs) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t seed[8];
  {
    const uint4* s4 = reinterpret_cast<const uint4*>(seeds + i * 32);
    const uint4 a = s4[0], b = s4[1];
    seed[0] = a.x; seed[1] = a.y; seed[2] = a.z; seed[3] = a.w;
    seed[4] = b.x; seed[5] = b.y; seed[6] = b.z; seed[7] = b.w;
  }
  const uint8_t* msg = msgs + i * (uint64_t)msg_len;
  uint32_t hs[16], dummy[8];
#pragma unroll
  for (int q = 0; q < 8; q++) dummy[q] = 0;
  sha512_segments(hs, seed, dummy, false, msg, 0);
  uint32_t a[8], prefix[8];
#pragma unroll
  for (int q = 0; q < 8; q++) {
    a[q] = hs[q];
    prefix[q] = hs[8 + q];
  }
  a[0] &= ~7u;
  a[7] &= 0x3fffffffu;
  a[7] |= 0x40000000u;
  uint32_t a16[16], ar[8];
#pragma unroll
  for (int q = 0; q < 8; q++) {
    a16[q] = a[q];
    a16[8 + q] = 0;
  }
  sc_reduce512(ar, a16);
  ge_p3 A;
  fixed_base_mult(A, ar, btab);
  uint32_t pub[8];
  ge_tobytes(pub, A);
  uint32_t rh[16], r[8];
  sha512_segments(rh, prefix, dummy, false, msg, msg_len);
  sc_reduce512(r, rh);
  ge_p3 Rp;
  fixed_base_mult(Rp, r, btab);
  uint32_t R[8];
  ge_tobytes(R, Rp);
  uint32_t kh[16], k[8], S[8];
  sha512_segments(kh, R, pub, true, msg, msg_len);
  sc_reduce512(k, kh);
  sc_muladd(S, k, ar, r);
  uint4* p4 = reinterpret_cast<uint4*>(pubs + i * 32);
  p4[0] = make_uint4(pub[0], pub[1], pub[2], pub[3]);
  p4[1] = make_uint4(pub[4], pub[5], pub[6], pub[7]);
  uint4* s4 = reinterpret_cast<uint4*>(sigs + i * 64);
  s4[0] = make_uint4(R[0], R[1], R[2], R[3]);
  s4[1] = make_uint4(R[4], R[5], R[6], R[7]);
  s4[2] = make_uint4(S[0], S[1], S[2], S[3]);
  s4[3] = make_uint4(S[4], S[5], S[6], S[7]);
}

}  // namespace cordahip

// ---------------------------------------------------------------------------
// host-side launchers (called by cordahip.cpp)
namespace cordahip {
hipError_t launch_ed25519_btable(uint32_t* tab, hipStream_t s) {
  hipLaunchKernelGGL(ed25519_btable_kernel, dim3((2 * kBTableEntries + 63) / 64), dim3(64), 0, s, tab);
  return hipGetLastError();
}
// the two tables and the identity entry behind them, padded to 256 B
size_t ed25519_btable_bytes() { return ((size_t)kBIdentityWord + 64) * sizeof(uint32_t); }

size_t ed25519_ws_lane_bytes() { return kWhLaneWords * sizeof(uint32_t); }

// Split verification, one prep/ladder launch pair per ws_lanes chunk (ws:
// ws_lanes * ed25519_ws_lane_bytes() of device memory, ws_lanes a multiple of
// 64; the caller orders the workspace's users). A missing workspace is an
// error: this is the only verification path.
hipError_t launch_ed25519_verify(const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                 uint64_t n, const uint32_t* btab, const uint8_t* pre_status, uint8_t* status,
                                 unsigned long long* verdict, uint32_t* ws, uint64_t ws_lanes, uint32_t flags,
                                 hipStream_t s, const std::function<hipError_t()>* before_msgs) {
  if (n == 0) return hipSuccess;
  if (!ws || ws_lanes < 64 || ws_lanes % 64) return hipErrorInvalidValue;
  bool msgs_ready = before_msgs == nullptr;
  for (uint64_t base = 0; base < n; base += ws_lanes) {
    const uint64_t m = n - base < ws_lanes ? n - base : ws_lanes;
    const uint32_t blocks = (uint32_t)((m + 255) / 256);
    hipError_t e = hipSuccess;
    if (msgs_ready) {
      hipLaunchKernelGGL(ed25519_prep_half_kernel, dim3(blocks), dim3(256), 0, s, keys, sigs, msgs, msg_len, base, m,
                         pre_status, status, ws, (flags & 1u) ? 0u : 1u);
      e = hipGetLastError();
    } else {
      // keys and R first; the messages' producer (enqueued by before_msgs on the same
      // stream) then runs beside this launch's tail, phase 2 after it
      hipLaunchKernelGGL(ed25519_prep_keys_kernel, dim3(blocks), dim3(256), 0, s, keys, sigs, msg_len, base, m,
                         pre_status, status, ws, (flags & 1u) ? 0u : 1u);
      e = hipGetLastError();
      e = e ? e : (*before_msgs)();
      msgs_ready = true;
      if (e == hipSuccess)
        hipLaunchKernelGGL(ed25519_prep_msg_kernel, dim3(blocks), dim3(256), 0, s, sigs, msgs, msg_len, base, m, status,
                           ws);
      e = e ? e : hipGetLastError();
    }
    if (e == hipSuccess) e = launch_ed25519_ladder(base, m, btab, ws, status, verdict, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The generic engine over the generic list of a routed batch of n lanes (scratch:
// ed25519_route.hpp): one fused-prep / ladder pair per ws_lanes list positions. The
// host does not know the list's length, so the pairs cover all n positions; the
// kernels read the count, and a pair wholly past it does nothing. No verdict words:
// the caller gathers them from the statuses. layout_lanes: the lanes the scratch was
// laid out for when that is not n (~0, runtime.hpp kEdIdxLayoutOfN: n; K23 passes 0, a
// header with the list right behind it).
hipError_t launch_ed25519_verify_idx(const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                     uint64_t n, const uint32_t* btab, const uint8_t* pre_status, uint8_t* status,
                                     uint32_t* ws, uint64_t ws_lanes, uint32_t flags, const uint32_t* scratch,
                                     hipStream_t s, uint64_t layout_lanes) {
  if (n == 0) return hipSuccess;
  const uint64_t lanes = layout_lanes == ~0ull ? n : layout_lanes;
  if (!ws || ws_lanes < 64 || ws_lanes % 64 || !scratch) return hipErrorInvalidValue;
  for (uint64_t base = 0; base < n; base += ws_lanes) {
    const uint64_t m = n - base < ws_lanes ? n - base : ws_lanes;
    const uint32_t blocks = (uint32_t)((m + 255) / 256);
    hipLaunchKernelGGL(ed25519_prep_half_idx_kernel, dim3(blocks), dim3(256), 0, s, keys, sigs, msgs, msg_len, base, m,
                       pre_status, status, ws, (flags & 1u) ? 0u : 1u, scratch, lanes);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = launch_ed25519_ladder_idx(base, m, btab, ws, status, scratch, lanes, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_ed25519_sign(const uint8_t* seeds, const uint8_t* msgs, uint32_t msg_len, uint64_t n,
                               const uint32_t* btab, uint8_t* pubs, uint8_t* sigs, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(ed25519_sign_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, seeds, msgs, msg_len, n, btab,
                     pubs, sigs);
  return hipGetLastError();
}
}  // namespace cordahip
