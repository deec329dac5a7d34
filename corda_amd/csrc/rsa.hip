// RSA_SHA256 (RSASSA-PSS, Crypto.kt:77-88) on the GPU: the public operation
// m = s^e mod n and the PSS checks (DESIGN §5 "RSA"; rules restated in
// rsa_key.hpp, PARITY UNPINNED).
//
// rsa_modexp_kernel<W>: W-word operands (W = 64 / 96 / 128: moduli of up to
// 2048 / 3072 / 4096 bits) do not fit one lane, so a GROUP of kT = 8 lanes holds
// one signature: lane g of the group keeps words [g L, (g + 1) L), L = W / kT,
// of the modulus, both operands and the accumulator in VGPRs. Montgomery
// multiplication is word-serial CIOS: for every word b_j (broadcast from its
// owner lane) each lane adds a_i b_j, then q n_i (q = t_0 n' from the group's
// low lane) into its window, and the accumulator moves down one word across
// the lanes. Carries out of a lane's window are kept in a per-lane `top` that
// rides along one position above the window (it is folded into the word that
// arrives from the next lane at every shift), so the inner loop has no
// cross-lane carry chain; the windows are normalised once per product.
// Per-key constants are derived per group on the device: n' by Newton steps,
// R^2 mod n by doubling 2^(bits - 1) up to 2^s R and squaring in Montgomery
// form (s 2^k = 32 W). The exponent runs left to right, wave-uniform in the
// bit position; every product of the kernel goes through ONE instance of the
// multiplication loop (a step schedule picks square / multiply and each group
// takes or discards the result), which keeps the code small.
//
// rsa_pss_prep_kernel / rsa_pss_check_kernel: one lane per signature; prep
// turns the big-endian signature into little-endian words and decides the
// statuses that need no arithmetic, check applies the PSS rules to m.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsa_route.hpp"
#include "rsa_sign.hpp"
#include "rsa_vkey.hpp"
#include "runtime.hpp"
#include "sha2_device.hpp"
#include "status.hpp"

namespace cordahip {
namespace {

constexpr int kT = 8;                      // lanes per signature
constexpr uint32_t kGroupMask = (1u << kT) - 1;
constexpr int kBlock = 256;                // 32 groups per block
constexpr int kGroupsPerBlock = kBlock / kT;

// this group's kT bits of a wave ballot
CDEV uint32_t group_bits(unsigned long long m, int gbase) { return (uint32_t)(m >> gbase) & kGroupMask; }

// t := t - n if ov (the word above the window of the top lane) or t >= n; t < 2 n
template <int L>
CDEV void cond_sub(uint32_t (&t)[L], const uint32_t (&n)[L], uint32_t ov, int gl, int gbase) {
  int c = 0;  // this window against the modulus', the higher word deciding
#pragma unroll
  for (int i = 0; i < L; i++) c = t[i] > n[i] ? 1 : t[i] < n[i] ? -1 : c;
  const uint32_t g = group_bits(__ballot(c > 0), gbase), l = group_bits(__ballot(c < 0), gbase);
  const bool sub = ov || g >= l;  // lanes are in order of significance: t >= n as integers of the windows' signs
  // borrow into each lane: a window below the modulus' generates, an equal one propagates
  const uint32_t a = (l | ~(g | l)) & kGroupMask, b = l;
  const uint32_t bin = (((a + b) ^ a ^ b) >> gl) & 1u;
  uint64_t br = bin;
#pragma unroll
  for (int i = 0; i < L; i++) {
    const uint64_t d = (uint64_t)t[i] - n[i] - br;
    br = (d >> 32) & 1u;
    t[i] = sub ? (uint32_t)d : t[i];
  }
}

// out = a b R^-1 mod n (R = 2^(32 L kT); a, b < n; n odd; np = -n^-1 mod 2^32)
template <int L>
CDEV void mont_mul(uint32_t (&out)[L], const uint32_t (&a)[L], const uint32_t (&b)[L], const uint32_t (&n)[L],
                   uint32_t np, int gl, int gbase) {
  uint32_t t[L];
#pragma unroll
  for (int i = 0; i < L; i++) t[i] = 0;
  uint64_t top = 0;  // carries out of the window: weight of word L
#pragma unroll 1
  for (int owner = 0; owner < kT; owner++) {
#pragma unroll
    for (int k = 0; k < L; k++) {
      const uint32_t bj = __shfl(b[k], owner, kT);
      uint64_t u = (uint64_t)a[0] * bj + t[0];
      t[0] = (uint32_t)u;
      uint32_t c = (uint32_t)(u >> 32);
      const uint32_t q = __shfl(t[0] * np, 0, kT);  // the group's low word decides q
#pragma unroll
      for (int i = 1; i < L; i++) {
        u = (uint64_t)a[i] * bj + t[i] + c;
        t[i] = (uint32_t)u;
        c = (uint32_t)(u >> 32);
      }
      top += c;
      u = (uint64_t)q * n[0] + t[0];
      const uint32_t t0 = (uint32_t)u;  // zero in the low lane; the word the lane below receives
      c = (uint32_t)(u >> 32);
#pragma unroll
      for (int i = 1; i < L; i++) {
        u = (uint64_t)q * n[i] + t[i] + c;
        t[i - 1] = (uint32_t)u;
        c = (uint32_t)(u >> 32);
      }
      top += c;
      uint32_t nx = __shfl_down(t0, 1, kT);
      if (gl == kT - 1) nx = 0;
      const uint64_t v = top + nx;
      t[L - 1] = (uint32_t)v;
      top = v >> 32;
    }
  }
  // normalise: each lane's pending carries into the lane above, until none is left
  // below the top lane (whose `top` is the word above the operand: 0 or 1)
  uint32_t tp = (uint32_t)top;
  while (__any(tp != 0 && gl != kT - 1)) {
    uint32_t cin = __shfl_up(tp, 1, kT);
    if (gl == 0) cin = 0;
    if (gl != kT - 1) tp = 0;
    uint64_t s = (uint64_t)t[0] + cin;
    t[0] = (uint32_t)s;
#pragma unroll
    for (int i = 1; i < L; i++) {
      s = (uint64_t)t[i] + (s >> 32);
      t[i] = (uint32_t)s;
    }
    tp += (uint32_t)(s >> 32);
  }
  cond_sub<L>(t, n, __shfl(tp, kT - 1, kT), gl, gbase);
#pragma unroll
  for (int i = 0; i < L; i++) out[i] = t[i];
}

// x = 2 x mod n (x < n)
template <int L>
CDEV void dbl_mod(uint32_t (&x)[L], const uint32_t (&n)[L], int gl, int gbase) {
  uint32_t below = __shfl_up(x[L - 1], 1, kT) >> 31;
  if (gl == 0) below = 0;
  const uint32_t ov = __shfl(x[L - 1] >> 31, kT - 1, kT);
#pragma unroll
  for (int i = L - 1; i > 0; i--) x[i] = (x[i] << 1) | (x[i - 1] >> 31);
  x[0] = (x[0] << 1) | below;
  cond_sub<L>(x, n, ov, gl, gbase);
}

// out[row] = in[row]^exp[row] mod mod[row], rows of W little-endian words. A row
// that breaks the contract (even or zero modulus, exp 0, in >= mod) or has a
// nonzero skip[row] gives a zero row and bad[row] = 1. in may alias out.
// kIdx (K20, the generic list of a routed launch): the grid covers the launch's rows and
// nrows is not used; the list's length is read from *count, a block wholly past it
// returns at once, as a block, and group j below it takes row perm[j] of the launch. The
// list holds rows the prep left OK only, so skip is not read. (K23's counted launch lists
// every row below its count: the packer sends only lanes whose key and lengths it has
// checked, so the prep leaves them OK but for a signature value >= n, which the contract
// check below turns into a zero row and bad[row] = 1 at no exponentiation's cost.)
// The two forms are instances of one kernel, as rsa_modexp_keyed_kernel's are
// (rsa_vkey.hip says why); both instances take the registers, LDS and waves per SIMD the
// kernel took before the template (70 / 97 / 130 VGPRs, 7 / 4 / 3 waves).
template <int W, bool kIdx>
__global__ void __launch_bounds__(kBlock) rsa_modexp_kernel(const uint32_t* __restrict__ mod,
                                                             const uint32_t* __restrict__ exp, const uint32_t* in,
                                                             uint64_t nrows, uint32_t* out, uint8_t* __restrict__ bad,
                                                             const uint8_t* __restrict__ skip,
                                                             const unsigned int* __restrict__ perm,
                                                             const unsigned int* __restrict__ count) {
  constexpr int L = W / kT;
  static_assert(W % kT == 0, "width class");
  if (kIdx) {
    nrows = *count;
    if (!rsa_route_idx_block_live(blockIdx.x, nrows)) return;
  }
  const int gl = threadIdx.x & (kT - 1);
  const int gbase = (threadIdx.x & 63) & ~(kT - 1);
  uint64_t row = (uint64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kT;
  // rows past the end and skipped rows load nothing and store nothing, and take
  // part in every cross-lane step with the stand-in operands below
  bool ok;
  if (kIdx) {
    ok = row < nrows;
    row = ok ? perm[row] : 0;
  } else {
    ok = row < nrows && !(skip && skip[row]);
  }
  const uint64_t base = row * W + (uint64_t)gl * L;
  uint32_t n[L], acc[L], other[L];
  uint32_t e = 1;
#pragma unroll
  for (int i = 0; i < L; i++) {
    n[i] = ok ? mod[base + i] : 0xffffffffu;
    other[i] = ok ? in[base + i] : 0u;
  }
  if (ok) e = exp[row];
  {
    // the contract: odd modulus, exponent >= 1, in < modulus
    int c = 0;
#pragma unroll
    for (int i = 0; i < L; i++) c = other[i] > n[i] ? 1 : other[i] < n[i] ? -1 : c;
    const uint32_t g = group_bits(__ballot(c > 0), gbase), l = group_bits(__ballot(c < 0), gbase);
    const uint32_t n0 = __shfl(n[0], 0, kT);
    const bool good = ok && (n0 & 1u) && e != 0 && g < l;
    if (!good) {  // stand-ins: n = R - 1, in = 0, e = 1
      e = 1;
#pragma unroll
      for (int i = 0; i < L; i++) {
        n[i] = 0xffffffffu;
        other[i] = 0;
      }
    }
    if (ok && gl == 0 && bad) bad[row] = good ? 0 : 1;
    if (ok && !good) {
#pragma unroll
      for (int i = 0; i < L; i++) out[base + i] = 0;
    }
    ok = good;
  }
  // n' = -n^-1 mod 2^32
  const uint32_t n0 = __shfl(n[0], 0, kT);
  uint32_t inv = n0;
#pragma unroll
  for (int k = 0; k < 5; k++) inv *= 2u - n0 * inv;
  const uint32_t np = 0u - inv;
  // bit length of the modulus
  uint32_t bits;
  {
    uint32_t hv = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < L; i++) {
      hi = n[i] ? (uint32_t)i : hi;
      hv = n[i] ? n[i] : hv;
    }
    const uint32_t nz = group_bits(__ballot(hv != 0), gbase);  // nonzero: the low lane's low word is odd
    const int toplane = 31 - __clz((int)nz);
    bits = __shfl(((uint32_t)gl * L + hi) * 32u + (32u - (uint32_t)__clz((int)hv)), toplane, kT);
  }
  // acc = 2^s R mod n by doubling 2^(bits - 1) (< n); s 2^sq = 32 W
  constexpr uint32_t kS = (32u * W) >> __builtin_ctz(32u * W), kSq = __builtin_ctz(32u * W);
#pragma unroll
  for (int i = 0; i < L; i++)
    acc[i] = ((uint32_t)gl * L + i == (bits - 1) >> 5) ? 1u << ((bits - 1) & 31) : 0u;
  const uint32_t nd = 32u * W + kS - (bits - 1);
  for (uint32_t k = 0; __any(k < nd); k++) {
    uint32_t x[L];
#pragma unroll
    for (int i = 0; i < L; i++) x[i] = acc[i];
    dbl_mod<L>(x, n, gl, gbase);
#pragma unroll
    for (int i = 0; i < L; i++) acc[i] = k < nd ? x[i] : acc[i];
  }
  // the wave's longest exponent sets the schedule
  uint32_t emax = e;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) emax = max(emax, (uint32_t)__shfl_xor((int)emax, off));
  const int topbit = 31 - __clz((int)__builtin_amdgcn_readfirstlane(emax));
  // steps: kSq squarings (acc = R^2), acc = acc * in (the base in Montgomery form;
  // `other` becomes the base), per exponent bit a square and a multiply, acc * 1
  const int first_bit = (int)kSq + 1, last = first_bit + 2 * (topbit + 1);
  bool started = false;
  for (int it = 0; it <= last; it++) {
    bool square = true, take = true;
    if (it == last) {
#pragma unroll
      for (int i = 0; i < L; i++) other[i] = (gl == 0 && i == 0) ? 1u : 0u;
    }
    if (it >= first_bit && it < last) {
      const int j = it - first_bit, bit = topbit - (j >> 1);
      const bool b = (e >> bit) & 1u;
      if (j & 1) {
        square = false;
        take = b && started;
        started = started || b;  // a group's first set bit: acc is the base already
      } else {
        take = started;
      }
      if (!__any(take)) continue;
    } else if (it >= first_bit - 1) {
      square = false;
    }
    uint32_t bsel[L], r[L];
#pragma unroll
    for (int i = 0; i < L; i++) bsel[i] = square ? acc[i] : other[i];
    mont_mul<L>(r, acc, bsel, n, np, gl, gbase);
#pragma unroll
    for (int i = 0; i < L; i++) acc[i] = take ? r[i] : acc[i];
    if (it == first_bit - 1) {
#pragma unroll
      for (int i = 0; i < L; i++) other[i] = acc[i];
    }
  }
  if (ok) {
#pragma unroll
    for (int i = 0; i < L; i++) out[base + i] = acc[i];
  }
}

// One lane per signature: the statuses that need no arithmetic (pre-status,
// UNSUPPORTED keys, EMPTY under doVerify rules, signatures longer than the
// modulus) and the signature as W little-endian words (zero for decided rows).
__global__ void __launch_bounds__(256) rsa_pss_prep_kernel(const uint32_t* __restrict__ mod,
                                                           const uint32_t* __restrict__ exp,
                                                           const uint8_t* __restrict__ sigs,
                                                           const uint16_t* __restrict__ sig_len,
                                                           const uint64_t* __restrict__ msg_off, uint32_t msg_len,
                                                           uint32_t W, uint64_t n, const uint8_t* __restrict__ pre,
                                                           uint32_t flags, uint32_t* __restrict__ words,
                                                           uint32_t* __restrict__ bits_out, uint8_t* __restrict__ st,
                                                           const unsigned int* __restrict__ count) {
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (count) n = *count;  // K23: the launch's rows are known on the device only
  if (row >= n) return;
  const uint32_t* m = mod + row * W;
  uint32_t bits = 0;
  for (uint32_t i = W; i-- > 0;) {
    const uint32_t v = m[i];
    if (v) {
      bits = i * 32 + (32 - (uint32_t)__clz((int)v));
      break;
    }
  }
  const uint32_t e = exp[row], sl = sig_len[row];
  const uint64_t ml = msg_off ? msg_off[row + 1] - msg_off[row] : msg_len;
  const uint32_t k = (bits + 7) / 8;
  uint8_t s = pre ? pre[row] : kStatusOk;
  if (s == kStatusOk) {
    if (!(m[0] & 1u) || bits < 1024 || bits > 32 * W || !(e & 1u) || e < 3) s = kStatusUnsupported;
    else if (!(flags & CORDAHIP_FLAG_IS_VALID) && (sl == 0 || ml == 0)) s = kStatusEmpty;
    else if (sl > k) s = kStatusBadSig;  // also every length beyond the slot: nothing past it is read
  }
  const uint8_t* sg = sigs + row * 4ull * W;
  uint32_t* w = words + row * W;
  for (uint32_t i = 0; i < W; i++) {
    uint32_t v = 0;
    if (s == kStatusOk) {
#pragma unroll
      for (uint32_t q = 0; q < 4; q++) {
        const uint32_t sig_byte = 4 * i + q;  // significance
        if (sig_byte < sl) v |= (uint32_t)sg[sl - 1 - sig_byte] << (8 * q);
      }
    }
    w[i] = v;
  }
  bits_out[row] = bits;
  st[row] = s;
}

// 32 bits of m starting at byte `off` of significance (little-endian), zero above W words
CDEV uint32_t m_bits32(const uint32_t* __restrict__ m, uint32_t W, uint32_t off) {
  const uint32_t i = off >> 2;
  const uint32_t lo = i < W ? m[i] : 0u, hi = i + 1 < W ? m[i + 1] : 0u;
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (off & 3)));
}

// One lane per signature: rules 3-8 on m = s^e mod n (rsa_key.hpp pss_check)
__global__ void __launch_bounds__(256) rsa_pss_check_kernel(const uint32_t* __restrict__ words,
                                                            const uint32_t* __restrict__ bits_in,
                                                            const uint8_t* __restrict__ st,
                                                            const uint8_t* __restrict__ bad,
                                                            const uint8_t* __restrict__ msgs,
                                                            const uint64_t* __restrict__ msg_off, uint32_t msg_len,
                                                            uint32_t W, uint64_t n, uint8_t* __restrict__ status,
                                                            unsigned long long* __restrict__ verdict,
                                                            const unsigned int* __restrict__ count) {
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (count) n = *count;  // K23, as in the prep
  uint8_t s = kStatusBadSig;
  if (row < n) {
    s = st[row];
    if (s == kStatusOk) {
      s = kStatusBadSig;
      const uint32_t* m = words + row * W;
      const uint32_t bits = bits_in[row], em_bits = bits - 1, em_len = (em_bits + 7) / 8, db_len = em_len - 33;
      bool good = !bad[row];
      // m < 2^(8 emLen), trailer 0xBC
      uint32_t above = m_bits32(m, W, em_len) ;
      for (uint32_t i = (em_len >> 2) + 1; i < W; i++) above |= m[i];
      good = good && above == 0 && (m[0] & 0xffu) == 0xbcu;
      if (good) {
        uint32_t H[8];
#pragma unroll
        for (int q = 0; q < 8; q++) H[q] = m_bits32(m, W, 29 - 4 * q);
        // DB = EM[0 .. dbLen) xor MGF1(H) as a stream of big-endian words; the last nine
        // of them hold the separator's neighbourhood and the salt
        const uint32_t sep = db_len - 33, ws = sep >> 2;
        const uint32_t zbits = 8 * em_len - em_bits;
        uint32_t lastw[9];
#pragma unroll
        for (int q = 0; q < 9; q++) lastw[q] = 0;
        uint32_t nz = 0;
        bool sep_ok = false;
        for (uint32_t ctr = 0; ctr * 32 < db_len; ctr++) {
          uint32_t h[8], w[16];
          sha256_init(h);
#pragma unroll
          for (int q = 0; q < 8; q++) w[q] = H[q];
          w[8] = ctr;
          w[9] = 0x80000000u;
#pragma unroll
          for (int q = 10; q < 15; q++) w[q] = 0;
          w[15] = 36 * 8;
          sha256_block(h, w);
#pragma unroll
          for (int q = 0; q < 8; q++) {
            const uint32_t j0 = ctr * 32 + 4 * q;
            if (j0 < db_len) {
              const uint32_t v = db_len - j0;  // bytes of this word inside DB
              const uint32_t keep = v >= 4 ? ~0u : ~0u << (32 - 8 * v);
              uint32_t d = (m_bits32(m, W, em_len - 4 - j0) ^ h[q]) & keep;
              if (j0 == 0) d &= 0xffffffffu >> zbits;  // cleared, not checked
              const uint32_t wi = j0 >> 2;
              if (wi < ws) nz |= d;
              if (wi == ws) sep_ok = (d >> (8 * (3 - (sep & 3)))) == 1u;
#pragma unroll
              for (int z = 0; z < 8; z++) lastw[z] = lastw[z + 1];
              lastw[8] = d;
            }
          }
        }
        const uint32_t r = (sep + 1) & 3;
        if (r == 0) {  // the salt starts on a word: align it as in the other cases
#pragma unroll
          for (int z = 0; z < 8; z++) lastw[z] = lastw[z + 1];
          lastw[8] = 0;
        }
        good = nz == 0 && sep_ok;
        if (good) {
          uint32_t salt[8];
#pragma unroll
          for (int q = 0; q < 8; q++)
            salt[q] = (uint32_t)(((((uint64_t)lastw[q]) << 32) | lastw[q + 1]) >> (32 - 8 * r));
          uint32_t mh[8], h[8], w[16];
          const uint64_t o = msg_off ? msg_off[row] : row * (uint64_t)msg_len;
          const uint64_t ml = msg_off ? msg_off[row + 1] - o : msg_len;
          sha256_bytes(mh, msgs + o, ml);
          sha256_init(h);
          w[0] = w[1] = 0;
#pragma unroll
          for (int q = 0; q < 8; q++) w[2 + q] = mh[q];
#pragma unroll
          for (int q = 0; q < 6; q++) w[10 + q] = salt[q];
          sha256_block(h, w);
          w[0] = salt[6];
          w[1] = salt[7];
          w[2] = 0x80000000u;
#pragma unroll
          for (int q = 3; q < 15; q++) w[q] = 0;
          w[15] = 72 * 8;
          sha256_block(h, w);
          uint32_t diff = 0;
#pragma unroll
          for (int q = 0; q < 8; q++) diff |= h[q] ^ H[q];
          if (diff == 0) s = kStatusOk;
        }
      }
    }
    status[row] = s;
  }
  const unsigned long long v = __ballot(row < n && s == kStatusOk);
  if (verdict && (threadIdx.x & 63) == 0 && row < n) verdict[row >> 6] = v;
}

template <int W>
hipError_t launch_modexp(const uint32_t* mod, const uint32_t* exp, const uint32_t* in, uint64_t n, uint32_t* out,
                         uint8_t* bad, const uint8_t* skip, hipStream_t s) {
  const uint64_t blocks = (n + kGroupsPerBlock - 1) / kGroupsPerBlock;
  hipLaunchKernelGGL((rsa_modexp_kernel<W, false>), dim3((uint32_t)blocks), dim3(kBlock), 0, s, mod, exp, in, n, out,
                     bad, skip, (const unsigned int*)nullptr, (const unsigned int*)nullptr);
  return hipGetLastError();
}

hipError_t modexp_any(uint32_t W, const uint32_t* mod, const uint32_t* exp, const uint32_t* in, uint64_t n,
                      uint32_t* out, uint8_t* bad, const uint8_t* skip, hipStream_t s) {
  switch (W) {
    case 64: return launch_modexp<64>(mod, exp, in, n, out, bad, skip, s);
    case 96: return launch_modexp<96>(mod, exp, in, n, out, bad, skip, s);
    case 128: return launch_modexp<128>(mod, exp, in, n, out, bad, skip, s);
  }
  return hipErrorInvalidValue;
}

// rows per launch: the grid's block count stays far below 2^31
constexpr uint64_t kMaxLaunchRows = 1ull << 24;

}  // namespace

uint32_t rsa_group_lanes() { return kT; }

hipError_t launch_rsa_public_op(const uint32_t* mod, const uint32_t* exp, const uint32_t* in, uint32_t W, uint64_t n,
                                uint32_t* out, hipStream_t s) {
  for (uint64_t lo = 0; lo < n; lo += kMaxLaunchRows) {
    const uint64_t m = std::min(kMaxLaunchRows, n - lo);
    hipError_t e = modexp_any(W, mod + lo * W, exp + lo, in + lo * W, m, out + lo * W, nullptr, nullptr, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// workspace per row: the signature / m words, the modulus' bit length, the
// pre-status and the modexp's contract flag
size_t rsa_ws_row_bytes(uint32_t W) { return 4ull * W + 4 + 2; }

hipError_t launch_rsa_pss_verify(const uint32_t* mod, const uint32_t* exp, const uint8_t* sigs,
                                 const uint16_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off,
                                 uint32_t msg_len, uint32_t W, uint64_t n, const uint8_t* pre, uint8_t* status,
                                 unsigned long long* verdict, uint8_t* ws, uint64_t ws_rows, uint32_t flags,
                                 hipStream_t s) {
  if (W != 64 && W != 96 && W != 128) return hipErrorInvalidValue;
  ws_rows = std::min(ws_rows, kMaxLaunchRows) / 64 * 64;  // launches start on verdict words
  if (n && !ws_rows) return hipErrorInvalidValue;
  uint32_t* words = reinterpret_cast<uint32_t*>(ws);
  uint32_t* bits = words + ws_rows * W;
  uint8_t* st = reinterpret_cast<uint8_t*>(bits + ws_rows);
  uint8_t* bad = st + ws_rows;
  for (uint64_t lo = 0; lo < n; lo += ws_rows) {
    const uint64_t m = std::min(ws_rows, n - lo);
    const dim3 grid((uint32_t)((m + 255) / 256));
    hipLaunchKernelGGL(rsa_pss_prep_kernel, grid, dim3(256), 0, s, mod + lo * W, exp + lo, sigs + lo * 4 * W,
                       sig_len + lo, msg_off ? msg_off + lo : nullptr, msg_len, W, m, pre ? pre + lo : nullptr, flags,
                       words, bits, st, (const unsigned int*)nullptr);
    hipError_t e = modexp_any(W, mod + lo * W, exp + lo, words, m, words, bad, st, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rsa_pss_check_kernel, grid, dim3(256), 0, s, words, bits, st, bad,
                       msg_off ? msgs : msgs + lo * msg_len, msg_off ? msg_off + lo : nullptr, msg_len, W, m,
                       status + lo, verdict ? verdict + lo / 64 : nullptr, (const unsigned int*)nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// K23: the same over rows whose number only the device knows (*count <= n, the host's
// upper bound; every row's pre-status is OK: the packer sent the decided lanes elsewhere).
// Per launch of the workspace loop a one-thread kernel leaves the launch's rows in
// launch_count[j]; the prep and the check return past it, and the exponentiation is the
// indexed instance (K20's, over iota: row j of the list is row j), whose blocks wholly
// past the count return as blocks. iota: at least min(ws_rows, n) words.
__global__ void rsa_launch_count_kernel(const unsigned int* __restrict__ count, uint64_t lo, uint64_t m,
                                        unsigned int* __restrict__ out) {
  *out = (unsigned int)rsa_route_launch_count(*count, lo, m);
}

template <int W>
static hipError_t launch_modexp_counted(const uint32_t* mod, const uint32_t* exp, uint32_t* words, uint64_t m,
                                        uint8_t* bad, const unsigned int* iota, const unsigned int* count,
                                        hipStream_t s) {
  hipLaunchKernelGGL((rsa_modexp_kernel<W, true>), dim3((uint32_t)rsa_route_idx_blocks(m)), dim3(kBlock), 0, s, mod,
                     exp, words, (uint64_t)0, words, bad, (const uint8_t*)nullptr, iota, count);
  return hipGetLastError();
}

static hipError_t modexp_counted_any(uint32_t W, const uint32_t* mod, const uint32_t* exp, uint32_t* words, uint64_t m,
                                     uint8_t* bad, const unsigned int* iota, const unsigned int* count,
                                     hipStream_t s) {
  switch (W) {
    case 64: return launch_modexp_counted<64>(mod, exp, words, m, bad, iota, count, s);
    case 96: return launch_modexp_counted<96>(mod, exp, words, m, bad, iota, count, s);
    case 128: return launch_modexp_counted<128>(mod, exp, words, m, bad, iota, count, s);
  }
  return hipErrorInvalidValue;
}

uint64_t rsa_counted_launches(uint64_t n, uint64_t ws_rows) {
  ws_rows = std::min(ws_rows, kMaxLaunchRows) / 64 * 64;
  return ws_rows ? (n + ws_rows - 1) / ws_rows : 0;
}

hipError_t launch_rsa_pss_verify_counted(const uint32_t* mod, const uint32_t* exp, const uint8_t* sigs,
                                         const uint16_t* sig_len, const uint8_t* msgs, uint32_t msg_len, uint32_t W,
                                         uint64_t n, const unsigned int* count, const unsigned int* iota,
                                         unsigned int* launch_count, uint8_t* status, uint8_t* ws, uint64_t ws_rows,
                                         uint32_t flags, hipStream_t s) {
  if (W != 64 && W != 96 && W != 128) return hipErrorInvalidValue;
  ws_rows = std::min(ws_rows, kMaxLaunchRows) / 64 * 64;
  if (n && (!ws_rows || !count || !iota || !launch_count)) return hipErrorInvalidValue;
  uint32_t* words = reinterpret_cast<uint32_t*>(ws);
  uint32_t* bits = words + ws_rows * W;
  uint8_t* st = reinterpret_cast<uint8_t*>(bits + ws_rows);
  uint8_t* bad = st + ws_rows;
  uint64_t j = 0;
  for (uint64_t lo = 0; lo < n; lo += ws_rows, j++) {
    const uint64_t m = std::min(ws_rows, n - lo);
    const dim3 grid((uint32_t)((m + 255) / 256));
    unsigned int* lc = launch_count + j;
    hipLaunchKernelGGL(rsa_launch_count_kernel, dim3(1), dim3(1), 0, s, count, lo, m, lc);
    hipLaunchKernelGGL(rsa_pss_prep_kernel, grid, dim3(256), 0, s, mod + lo * W, exp + lo, sigs + lo * 4 * W,
                       sig_len + lo, (const uint64_t*)nullptr, msg_len, W, m, (const uint8_t*)nullptr, flags, words,
                       bits, st, (const unsigned int*)lc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = modexp_counted_any(W, mod + lo * W, exp + lo, words, m, bad, iota, lc, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rsa_pss_check_kernel, grid, dim3(256), 0, s, words, bits, st, bad, msgs + lo * msg_len,
                       (const uint64_t*)nullptr, msg_len, W, m, status + lo, (unsigned long long*)nullptr,
                       (const unsigned int*)lc);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// K18, verification against registered keys: the kernels share this unit's device
// functions (none of them changes; the generic kernels compile as before)
#include "rsa_vkey.hip"

// K20, routing of rows to K18's exponentiation on the GPU: the route pass and the launch
// parts of a routed batch
#include "rsa_route.hip"

// K19, signing with registered private keys: shares the group layout and SHA-256; its
// Montgomery product is a constant-time variant of its own
#include "rsa_sign_keyed.hip"

}  // namespace cordahip
