// Selector stream of the Ed25519 ladder: what the prep leaves in the record's 32
// scalar words instead of |c0|, c1 and e themselves, so that the ladder's
// window front end is one LDS read, a bit-field extract and an address.
//
//   words  0 .. 21  one 5-bit selector per joint window j (field j % 6 of word
//                   j / 6): bits 0 .. 3 the entry index 0 .. 11 of
//                   joint_select(joint_booth2(|c0|, j), joint_booth2(c1, j), c0neg)
//                   (ed25519_joint.hpp) or kSelIdentity for the digit pair (0, 0),
//                   bit 4 (kSelNeg) set when the window adds the entry's negative.
//                   The digits past a scalar's last window are zero, so the
//                   windows at or above the lane's own count select the identity.
//   words 22 ..     the kBDigits fixed-base Booth digits of e of width kBBits
//                   (ED_B_BITS: 20, 18 or 16): kBDigitsLo over B, then kBDigitsHi
//                   over B' = [2^(kBDigitsLo kBBits)]B, as magnitudes
//                   0 .. 2^(kBBits - 1), one bit string of kBBits-bit fields:
//                   digit t at bit kBBits t of the kSelMagWords words (9, 9, 8;
//                   at width 16 that is half t & 1 of word 22 + (t >> 1))
//   word kSelMeta   (31, 31, 30) bit t: digit t is negative; bits 16 .. 23: the
//                   lane's window count (bitlen(max(|c0|, c1)) + 2) / 2
//
// The number of fixed-base additions is the number of digits, ceil(254 / kBBits)
// (e < 2^253 and the Booth carry), whatever the tables cost: 13 at width 20 (7 + 6),
// 15 at 18 (8 + 7), 16 at 16 (8 + 8). The low digits end at the ladder's window
// (kBDigitsLo - 1) kBBits / 2, which has to be a window every lane has anyway
// (64 of them: |c0|, c1 ~ 2^128), hence the uneven splits.
//
// 132 windows, because the scalars are not always half-size: |c0|, c1 < 8L <
// 2^256 need up to 129. Where Euclid's short vector has an even c1 the prep
// takes the shortest of six neighbours with an odd c1 (half_choose,
// ed25519_half.hpp): the next Euclid vector, whose length is 8L over the short
// one's remainder, or the previous one, which is short when that one is long.
// By the CPU model (tools/proto/half_scalar_windows.py; not a GPU measurement)
// about one lane in 5,000 needs 68 windows or more (one in 120 while only the
// next vector's three were tried) and the longest of 200,000 needs 69 (73), but
// nothing bounds it below 129: h = L - 1 gives 252 bits. Windows 80 and up are recoded only for a lane that has a bit
// at or above 159 (one branch); every other position is a compile-time
// constant once the loops are unrolled: no dynamic shift. Usable from host and
// device (tests/test_ed_sel_recode.py builds tools/ed_sel_check.cpp from it).
#pragma once
#include <stdint.h>

#include "ed25519_joint.hpp"

namespace cordahip {

static constexpr int kSelPerWord = 6, kSelBits = 5;
static constexpr int kSelWindows = 132;                       // >= 129, whole words
static constexpr uint32_t kSelIdentity = 15;
static constexpr uint32_t kSelNeg = 16;
// width of the fixed-base Booth windows over e: a multiple of the ladder's 2-bit
// window, so both share the doublings
#ifndef ED_B_BITS
#define ED_B_BITS 20
#endif
static constexpr int kBBits = ED_B_BITS;
static_assert(kBBits == 16 || kBBits == 18 || kBBits == 20, "ED_B_BITS: 16, 18 or 20");
static constexpr int kBWin = kBBits / 2;                      // ladder windows per fixed-base window
static constexpr int kBDigitsLo = 63 / kBWin + 1;             // over B: 8, 8, 7
static constexpr int kBDigitsHi = (254 + kBBits - 1) / kBBits - kBDigitsLo;  // over B': 8, 7, 6
static constexpr int kBDigits = kBDigitsLo + kBDigitsHi;
static constexpr int kBMinWindows = (kBDigitsLo - 1) * kBWin + 1;  // the low digits' top window, counted
static_assert(kBDigits * kBBits >= 254, "e < 2^253 and the Booth carry");
static_assert(kBMinWindows <= 64, "the digits force no window a normal lane does not have");
static_assert(kBDigitsHi >= 1 && kBDigitsHi <= kBDigitsLo, "a window's high digit has a low digit beside it");
static constexpr int kSelMag = kSelWindows / kSelPerWord;     // word of the first magnitude
static constexpr int kSelMagWords = (kBDigits * kBBits + 31) / 32;
static constexpr int kSelMeta = kSelMag + kSelMagWords;       // signs and window count
static constexpr int kSelWords = kSelMeta + 1;                // 32 (width 16: 31)
static_assert(kBDigits <= 16, "the meta word's sign bits");
static constexpr int kSelAlways = 80;                         // windows recoded for every lane: scalar words 0 .. 4
static_assert(kSelWindows % kSelPerWord == 0 && kSelWindows >= 129 && kSelWords <= 32,
              "the stream lives in the record's 32 scalar words");

// d + 2 for the Booth digit d = b_lo + b_mid - 2 b_hi of the three bits v
// (joint_booth2's last line), three bits per entry: v = 0 .. 7 -> 0 1 1 2 -2 -1 -1 0
static constexpr uint32_t kBooth2Lut = 2u | 3u << 3 | 3u << 6 | 4u << 9 | 0u << 12 | 1u << 15 | 1u << 18 | 2u << 21;

// the selector of the window whose bit triples are va (of |c0|, already
// complemented when c0 < 0: see sel_recode) and vr (of c1). With s = 5 da + dr
// (|dr| <= 2 < 5, so s orders the pairs as joint_select does): the window adds
// the negative iff s < 0, and the entry is joint_index(|da|, +-dr) = |s| - 1,
// which is -1 = kJointIdentity for the pair (0, 0).
JOINT_HD uint32_t sel_byte(uint32_t va, uint32_t vr) {
  const int ta = (int)((kBooth2Lut >> (3 * va)) & 7u), tr = (int)((kBooth2Lut >> (3 * vr)) & 7u);
  const int s = 5 * ta + tr - 12;
  const int m = s < 0 ? -s : s;
  return ((uint32_t)(m - 1) & 15u) | (s < 0 ? kSelNeg : 0u);
}
static_assert(((uint32_t)kJointIdentity & 15u) == kSelIdentity && kJointEntries <= (int)kSelIdentity &&
                  (kSelNeg | 15u) < (1u << kSelBits),
              "selector encoding");

// Window j = 16 w + b of a scalar reads the bits 2b - 1 .. 2b + 1 of its word w
// (b = 0: the top bit of word w - 1 and two bits), so a word yields its 16
// triples with constant shifts. Negating every digit of |c0| (c0 < 0: the ladder
// then adds [|c0|]A) is complementing every bit, the implicit bit -1 included:
// b'_lo + b'_mid - 2 b'_hi = -(b_lo + b_mid - 2 b_hi).
//
// the 16 windows of scalar word w (a of |c0|, complemented for c0 < 0; r of c1;
// pa, pr: the bits below them) into their fields, which hold zero or, from
// kSelAlways up, the identity
JOINT_HD void sel_word(uint32_t out[kSelWords], int w, uint32_t a, uint32_t r, uint32_t pa, uint32_t pr) {
#pragma unroll
  for (int b = 0; b < 16; b++) {
    const int j = 16 * w + b;
    if (j >= kSelWindows) break;
    const uint32_t va = b ? (a >> (2 * b - 1)) & 7u : ((a << 1) | pa) & 7u;
    const uint32_t vr = b ? (r >> (2 * b - 1)) & 7u : ((r << 1) | pr) & 7u;
    const int sh = kSelBits * (j % kSelPerWord);
    out[j / kSelPerWord] ^= (sel_byte(va, vr) ^ (j >= kSelAlways ? kSelIdentity : 0u)) << sh;
  }
}

JOINT_HD void sel_recode(uint32_t out[kSelWords], const uint32_t c0abs[8], const uint32_t c1[8], const uint32_t e[8],
                         bool c0neg) {
  const uint32_t flip = c0neg ? ~0u : 0u;
#pragma unroll
  for (int k = 0; k < kSelMag; k++) {
    uint32_t v = 0;
#pragma unroll
    for (int t = 0; t < kSelPerWord; t++)
      if (kSelPerWord * k + t >= kSelAlways) v |= kSelIdentity << (kSelBits * t);
    out[k] = v;
  }
#pragma unroll
  for (int w = 0; w < kSelAlways / 16; w++)
    sel_word(out, w, c0abs[w] ^ flip, c1[w], w ? (c0abs[w - 1] ^ flip) >> 31 : flip >> 31, w ? c1[w - 1] >> 31 : 0u);
  // a digit of a window from kSelAlways up is non-zero only with a bit at or above 2 kSelAlways - 1 set
  const uint32_t high = (c0abs[4] | c1[4]) >> 31 | c0abs[5] | c1[5] | c0abs[6] | c1[6] | c0abs[7] | c1[7];
  if (high) {
#pragma unroll
    for (int w = kSelAlways / 16; w <= 8; w++)
      sel_word(out, w, (w < 8 ? c0abs[w] : 0u) ^ flip, w < 8 ? c1[w] : 0u, (c0abs[w - 1] ^ flip) >> 31, c1[w - 1] >> 31);
  }
  // fixed-base digits of width kBBits (sc25519.hpp booth_digit<kBBits>): digit t
  // reads the bits kBBits t - 1 .. kBBits t + kBBits - 1 (bit -1 and the bits
  // from 256 up are zero), every position a constant
  uint32_t signs = 0;
#pragma unroll
  for (int w = 0; w < kSelMagWords; w++) out[kSelMag + w] = 0;
#pragma unroll
  for (int t = 0; t < kBDigits; t++) {
    const int lo = kBBits * t - 1, w = lo < 0 ? 0 : lo >> 5, sh = lo < 0 ? 0 : lo & 31;
    uint32_t v = lo < 0 ? e[0] << 1 : e[w] >> sh;
    if (sh && w + 1 < 8) v |= e[w + 1] << (32 - sh);
    v &= (2u << kBBits) - 1;
    const int d = (int)((v + 1) >> 1) - (int)((v >> kBBits) << kBBits);
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
    signs |= (d < 0 ? 1u : 0u) << t;
    const int ow = (kBBits * t) >> 5, osh = (kBBits * t) & 31;
    out[kSelMag + ow] |= mag << osh;
    if (osh + kBBits > 32) out[kSelMag + ow + 1] |= mag >> (32 - osh);
  }
  // bitlen(max(|c0|, c1)) is the bit length of their OR
  int bits = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint32_t m = c0abs[i] | c1[i];
    bits = m ? 32 * i + 32 - __builtin_clz(m) : bits;
  }
  out[kSelMeta] = signs | (uint32_t)((bits + 2) / 2) << 16;  // at most 129
}

// the fields as the ladder reads them
JOINT_HD uint32_t sel_window(const uint32_t s[kSelWords], int j) {
  return (s[j / kSelPerWord] >> (kSelBits * (j % kSelPerWord))) & ((1u << kSelBits) - 1);
}
JOINT_HD int sel_count(const uint32_t s[kSelWords]) { return (int)((s[kSelMeta] >> 16) & 0xffu); }
// magnitude of fixed-base digit t of a stream whose word w is s[w * stride] (the
// ladder keeps it word-major in LDS): the field may straddle two words; the word
// behind the last field's first is at most the meta word
JOINT_HD uint32_t sel_bmag(const uint32_t* s, int stride, int t) {
  const int w = kSelMag + ((kBBits * t) >> 5), sh = (kBBits * t) & 31;
  const uint64_t two = (uint64_t)s[(w + 1) * stride] << 32 | s[w * stride];
  return (uint32_t)(two >> sh) & ((1u << kBBits) - 1);
}
JOINT_HD bool sel_bneg(uint32_t meta, int t) { return (meta >> t) & 1u; }
JOINT_HD int sel_bdigit(const uint32_t s[kSelWords], int t) {
  const int mag = (int)sel_bmag(s, 1, t);
  return sel_bneg(s[kSelMeta], t) ? -mag : mag;
}

}  // namespace cordahip
