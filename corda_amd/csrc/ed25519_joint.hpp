// Joint 2-bit Booth recoding of the Ed25519 ladder's two per-lane scalars.
//
// The ladder adds [c0](+-A) + [c1](-R) with one addition per 2-bit window: the
// digits (da, dr) of the two scalars, each in [-2, 2], select one entry
// i P + j Q of a per-lane table over P = -A, Q = -R. Of the 24 non-zero pairs
// only the 12 with i > 0, or i == 0 and j > 0, are stored; the others are
// their negatives (a swap and a sign in cached form), and (0, 0) is the shared
// identity. Usable from host and device (tests/test_ed_joint_recode.py builds
// tools/ed_joint_check.cpp from it).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JOINT_HD __host__ __device__ inline
#else
#define JOINT_HD inline
#endif

namespace cordahip {

static constexpr int kJointEntries = 12;
static constexpr int kJointIdentity = -1;

// Booth digit j of width 2 of the little-endian scalar k[0 .. nwords) (word w
// at k[w * stride]; bits past the last word are zero):
//   d_j = b_{2j-1} + b_{2j} - 2 b_{2j+1}  in [-2, 2],  sum_j d_j 4^j = k
// over the digits j < (bitlen(k) + 2) / 2. Digit positions are the same in
// every lane, so the ladder never diverges.
JOINT_HD int joint_booth2(const uint32_t* k, int stride, int nwords, int j) {
  const int lo = 2 * j - 1;  // may be -1
  uint32_t v;
  if (lo < 0) {
    v = (k[0] << 1) & 7u;
  } else {
    const int w = lo >> 5, sh = lo & 31;
    const uint64_t l = w < nwords ? k[w * stride] : 0u;
    const uint64_t h = w + 1 < nwords ? k[(w + 1) * stride] : 0u;
    v = (uint32_t)(((h << 32) | l) >> sh) & 7u;
  }
  return (int)((v + 1) >> 1) - (int)((v >> 2) << 2);
}

// index of the stored entry i P + j Q (i > 0, or i == 0 and j > 0):
//   (0,1) (0,2) | (1,-2) .. (1,2) | (2,-2) .. (2,2)  ->  0 1 | 2 .. 6 | 7 .. 11
JOINT_HD constexpr int joint_index(int i, int j) { return 5 * i + j - 1; }

struct joint_sel {
  int idx;   // 0 .. 11, or kJointIdentity
  bool neg;  // the window adds -(entry idx)
};

// the entry the window with digits (da, dr) adds: da P' + dr Q, P' = -P when
// c0neg ([c0](-A) with c0 < 0 is [|c0|]A: da's sign flips first)
JOINT_HD joint_sel joint_select(int da, int dr, bool c0neg) {
  da = c0neg ? -da : da;
  joint_sel s;
  s.neg = da < 0 || (da == 0 && dr < 0);
  const int i = s.neg ? -da : da, j = s.neg ? -dr : dr;
  s.idx = joint_index(i, j);  // (0, 0) -> -1 == kJointIdentity
  return s;
}

}  // namespace cordahip
