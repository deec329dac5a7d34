// RSA_SHA256 signing with registered private keys (K19): part of rsa.hip's translation
// unit, whose kT-lane group layout and SHA-256 it shares (none of K8's or K18's code
// changes; their kernels compile as before). The record, the schedule, its bounds and
// the host reference are in rsa_sign.hpp.
//
// rsa_sign_prep_kernel: one lane per signature decides the statuses that need no
// arithmetic (SKIPPED, UNKNOWN_KEY, EMPTY) and builds EM = EMSA-PSS-ENCODE(m, salt) as W
// little-endian words. Nothing here is secret: EM is s^e mod n, which every verifier
// computes.
//
// rsa_sign_keyed_kernel<W>: a group of kT = 8 lanes per signature, 8 groups a block.
// The group runs the two half exponentiations EM^dP mod p and EM^dQ mod q in turn at
// H = W / 16 words a lane, recombines them (Garner), widens to L = W / 8 words a lane
// for q h and the fault check s^e mod n == EM (K18's chain), and writes the signature
// as k big-endian bytes. A lane that fails the check answers SIGN_FAILED with a zero
// slot.
//
// Constant time by construction. Secrets are p, q, dP, dQ, qInv, every window digit,
// every table entry, m1, m2, h and every intermediate mod p or mod q. For them
//   1. no loop bound depends on operand values: mont_mul_ct normalises its windows in
//      kT - 1 rounds (carry_norm_ct proves the count) where mont_mul loops on __any;
//   2. no step is skipped on a digit: every window is kSignWin squarings and one product
//      with a table entry (entry 0 for digit 0); the windows cover the wave's longest
//      ceil(pbits / 32) exponent words, pbits the record's public prime bit length;
//   3. a window's entry is chosen without a secret address: all 2^kSignWin entries are
//      read from LDS (addresses: the loop counter and the thread index) and the lane's
//      own kept by masks that are opaque to the optimizer (sign_mask);
//   4. the conditional subtractions (cond_sub_ct), the comparison before them (cmp_ct)
//      and the sign fix of m1 - m2 (add_masked_ct) end in selects by such masks.
// __ballot of a secret comparison yields a scalar value, never a branch: the borrow
// lookahead is arithmetic on it. What does branch is public: the prep status (gate,
// message length), the key id and class against the record, the lane index inside the
// group, e (the fault check's schedule, K18's) and the outcome of the fault check.
//
// The window table lives in LDS, each lane's words in a column of its own
// (tl[entry][word][thread]): no lane reads another's, no barrier is needed, and
// consecutive lanes read consecutive banks. 2^3 * H * 4 B a lane: 8 / 12 / 16 KiB a
// 64-thread block (static_assert below: at most 64 KiB). The kernel zeroes its columns before it ends; no secret is written
// to HBM (m1, m2 and h stay in registers).
// No group returns before a shuffle: a row past the end, decided by the prep, of an
// unknown key or of another class loads nothing of any key and runs every cross-lane
// step on stand-ins (x = Rp - 1, x' = 1, Rp^2 mod x = 1, EM = 0, exponent 0; n = R - 1,
// n' = 1, qR = 0, e = 1, K = 1).

namespace {

// threads a block: 64 ships (DESIGN.md K19 has the A/B; -DCORDAHIP_RSA_SIGN_BLOCK=b measures another)
#ifndef CORDAHIP_RSA_SIGN_BLOCK
#define CORDAHIP_RSA_SIGN_BLOCK 64
#endif
constexpr int kSignBlock = CORDAHIP_RSA_SIGN_BLOCK;  // 8 groups
static_assert(kSignBlock % 64 == 0 && kSignBlock <= 256, "whole waves");
constexpr int kSignGroups = kSignBlock / kT;
constexpr int kSignEntries = 1 << rsa::kSignWin;

// All ones when c holds, else zero, behind an empty asm: the optimizer sees an opaque
// word, so a selection written with it stays AND / OR arithmetic and cannot be turned
// back into control flow on the (secret) condition.
CDEV uint32_t sign_mask(bool c) {
  uint32_t m = 0u - (uint32_t)c;
  asm volatile("" : "+v"(m));
  return m;
}
CDEV uint32_t sign_sel(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }  // m ? a : b

// Each lane's pending carries tp (weight: the word above its window) into the lane
// above, in kT - 1 rounds. A round hands every tp of a lane below the top one up and
// leaves there the carry out of its own window. Lane 0 receives nothing, so after round
// 1 its tp is 0 for good; lane g receives in round r only what lane g - 1 held after
// round r - 1, so by induction tp_g = 0 after round g + 1 and stays 0: after kT - 1
// rounds no lane below the top one holds a carry. The top lane accumulates: its tp is
// the word above the operand.
template <int L>
CDEV void carry_norm_ct(uint32_t (&t)[L], uint32_t& tp, int gl) {
#pragma unroll 1
  for (int r = 0; r < kT - 1; r++) {
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
}

// this group's ballots of "window a > window b" and "window a < window b", by arithmetic
template <int L>
CDEV void cmp_ct(const uint32_t (&a)[L], const uint32_t (&b)[L], int gbase, uint32_t& g, uint32_t& l) {
  uint32_t cg = 0, cl = 0;  // the higher word decides
#pragma unroll
  for (int i = 0; i < L; i++) {
    const uint32_t gt = (uint32_t)(((uint64_t)b[i] - a[i]) >> 63), lt = (uint32_t)(((uint64_t)a[i] - b[i]) >> 63);
    const uint32_t keep = (gt | lt) ^ 1u;
    cg = gt | (cg & keep);
    cl = lt | (cl & keep);
  }
  g = group_bits(__ballot(cg != 0), gbase);
  l = group_bits(__ballot(cl != 0), gbase);
}

// d = a - b mod 2^(32 L kT); all ones when a < b (it borrowed), else zero
template <int L>
CDEV uint32_t sub_ct(uint32_t (&d)[L], const uint32_t (&a)[L], const uint32_t (&b)[L], int gl, int gbase) {
  uint32_t g, l;
  cmp_ct<L>(a, b, gbase, g, l);
  // borrow into each lane: a window below the other's generates, an equal one propagates
  const uint32_t pa = (l | ~(g | l)) & kGroupMask, pb = l;
  uint64_t br = (((pa + pb) ^ pa ^ pb) >> gl) & 1u;
#pragma unroll
  for (int i = 0; i < L; i++) {
    const uint64_t v = (uint64_t)a[i] - b[i] - br;
    br = (v >> 32) & 1u;
    d[i] = (uint32_t)v;
  }
  return sign_mask(l > g);  // lanes are in order of significance
}

// t := t - n if ov (the word above the window of the top lane) or t >= n, by mask; t < 2 n
template <int L>
CDEV void cond_sub_ct(uint32_t (&t)[L], const uint32_t (&n)[L], uint32_t ov, int gl, int gbase) {
  uint32_t d[L];
  const uint32_t below = sub_ct<L>(d, t, n, gl, gbase);
  const uint32_t m = sign_mask(ov != 0) | ~below;
#pragma unroll
  for (int i = 0; i < L; i++) t[i] = sign_sel(m, d[i], t[i]);
}

// t := t + (x & m) mod 2^(32 L kT), m a mask word
template <int L>
CDEV void add_masked_ct(uint32_t (&t)[L], const uint32_t (&x)[L], uint32_t m, int gl) {
  uint64_t s = 0;
#pragma unroll
  for (int i = 0; i < L; i++) {
    s = (uint64_t)t[i] + (x[i] & m) + (s >> 32);
    t[i] = (uint32_t)s;
  }
  uint32_t tp = (uint32_t)(s >> 32);
  carry_norm_ct<L>(t, tp, gl);
}

// out = a b R^-1 mod n (R = 2^(32 L kT); n odd; np = -n^-1 mod 2^32) for a b < R n: one
// operand below n, the other merely below R (rsa_sign.hpp: the running sum stays below
// R + n, one bit above the windows, and the result below 2 n before the subtraction).
// mont_mul's loop with a fixed-round normalise and a masked subtraction.
template <int L>
CDEV void mont_mul_ct(uint32_t (&out)[L], const uint32_t (&a)[L], const uint32_t (&b)[L], const uint32_t (&n)[L],
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
  uint32_t tp = (uint32_t)top;
  carry_norm_ct<L>(t, tp, gl);
  cond_sub_ct<L>(t, n, __shfl(tp, kT - 1, kT), gl, gbase);
#pragma unroll
  for (int i = 0; i < L; i++) out[i] = t[i];
}

// the record of the lane's signing key if it is live in class W, else null: the slot's
// index word is a hint, the record's id and class decide
CDEV const uint32_t* rsa_sign_record(const uint32_t* __restrict__ tab, uint32_t id, uint32_t W) {
  if (!tab) return nullptr;
  const uint32_t ix = tab[rsa::kSignTabIdxWord + (id & (rsa::kSignSlots - 1))];
  if (ix == 0 || ix > rsa::kSignerMaxKeys) return nullptr;
  const uint32_t* rec = tab + rsa::kSignTabRecBase + (size_t)(ix - 1) * rsa::kSignRecWords;
  return (rec[rsa::kSignRecIdWord] == id && rec[rsa::kSignRecWordsWord] == W) ? rec : nullptr;
}

// One lane per signature: the status (SKIPPED, UNKNOWN_KEY for a key that is not live in
// class W, EMPTY, else OK) and EM as W little-endian words (zero for decided rows). Only
// the record's id, class and bit length are read.
__global__ void __launch_bounds__(256) rsa_sign_prep_kernel(const uint32_t* __restrict__ tab,
                                                            const uint32_t* __restrict__ key_id,
                                                            const uint8_t* __restrict__ msgs,
                                                            const uint64_t* __restrict__ msg_off, uint32_t msg_len,
                                                            const uint8_t* __restrict__ salts,
                                                            const uint8_t* __restrict__ gate, uint32_t W, uint64_t n,
                                                            uint32_t* __restrict__ words, uint8_t* __restrict__ st) {
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const uint64_t o = msg_off ? msg_off[row] : row * (uint64_t)msg_len;
  const uint64_t ml = msg_off ? msg_off[row + 1] - o : msg_len;
  uint8_t s = kStatusOk;
  const uint32_t* rec = nullptr;
  if (gate && gate[row]) s = kSignSkipped;
  else if (!(rec = rsa_sign_record(tab, key_id[row], W))) s = kSignUnknownKey;
  else if (ml == 0) s = kStatusEmpty;
  st[row] = s;
  uint32_t* w = words + row * W;
  for (uint32_t i = 0; i < W; i++) w[i] = 0;
  if (s != kStatusOk) return;
  const uint32_t bits = rec[rsa::kSignRecBitsWord];  // 1024 .. 32 W
  const uint32_t em_bits = bits - 1, em_len = (em_bits + 7) / 8, db_len = em_len - 33, zbits = 8 * em_len - em_bits;
  uint8_t* wb = reinterpret_cast<uint8_t*>(w);  // byte of significance b at wb[b]; em_len <= 4 W
  const uint8_t* salt = salts + row * 32;
  uint32_t sw[8], mh[8], H[8], wk[16];
#pragma unroll
  for (int q = 0; q < 8; q++)
    sw[q] = (uint32_t)salt[4 * q] << 24 | (uint32_t)salt[4 * q + 1] << 16 | (uint32_t)salt[4 * q + 2] << 8 |
            salt[4 * q + 3];
  sha256_bytes(mh, msgs + o, ml);
  // H = SHA-256(0x00 * 8 || mHash || salt): 72 bytes, two blocks
  sha256_init(H);
  wk[0] = wk[1] = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) wk[2 + q] = mh[q];
#pragma unroll
  for (int q = 0; q < 6; q++) wk[10 + q] = sw[q];
  sha256_block(H, wk);
  wk[0] = sw[6];
  wk[1] = sw[7];
  wk[2] = 0x80000000u;
#pragma unroll
  for (int q = 3; q < 15; q++) wk[q] = 0;
  wk[15] = 72 * 8;
  sha256_block(H, wk);
  wb[0] = 0xbc;
#pragma unroll
  for (int q = 0; q < 8; q++) {
#pragma unroll
    for (int z = 0; z < 4; z++) wb[1 + 31 - (4 * q + z)] = (uint8_t)(H[q] >> (24 - 8 * z));
  }
  // DB = 0x00 .. || 0x01 || salt, xor MGF1(H): DB[j] has significance em_len - 1 - j
  for (uint32_t ctr = 0; ctr * 32 < db_len; ctr++) {
    uint32_t h[8];
    sha256_init(h);
#pragma unroll
    for (int q = 0; q < 8; q++) wk[q] = H[q];
    wk[8] = ctr;
    wk[9] = 0x80000000u;
#pragma unroll
    for (int q = 10; q < 15; q++) wk[q] = 0;
    wk[15] = 36 * 8;
    sha256_block(h, wk);
#pragma unroll
    for (int q = 0; q < 8; q++) {
#pragma unroll
      for (int z = 0; z < 4; z++) {
        const uint32_t j = ctr * 32 + 4 * q + z;
        if (j < db_len) {
          uint32_t v = (h[q] >> (24 - 8 * z)) & 0xffu;
          if (j + 33 == db_len) v ^= 1u;
          else if (j + 32 >= db_len) v ^= salt[j + 32 - db_len];
          if (j == 0) v &= 0xffu >> zbits;
          wb[em_len - 1 - j] = (uint8_t)v;
        }
      }
    }
  }
}

// a half-width operand (H words a lane, below 2^(32 H kT)) in the full-width layout
// (2 H words a lane): lane g takes the windows of half lanes 2 g and 2 g + 1, the upper
// four lanes zero
template <int H>
CDEV void sign_widen(uint32_t (&f)[2 * H], const uint32_t (&h)[H], int gl) {
#pragma unroll
  for (int i = 0; i < H; i++) {
    const uint32_t a = __shfl(h[i], (2 * gl) & (kT - 1), kT), b = __shfl(h[i], (2 * gl + 1) & (kT - 1), kT);
    f[i] = gl < kT / 2 ? a : 0u;
    f[H + i] = gl < kT / 2 ? b : 0u;
  }
}

// acc = EM^exp mod x in Montgomery form (rsa_sign.hpp half_exp): x, r2 = Rp^2 mod x and
// the exponent from the record (null: the stand-ins), EM's halves from `em` (null: zero),
// nwords exponent words (wave-uniform). tl: the block's window table.
template <int H>
CDEV void sign_half_exp(uint32_t (&acc)[H], const uint32_t* __restrict__ xw, const uint32_t* __restrict__ r2w,
                        const uint32_t* __restrict__ expw, uint32_t npx, const uint32_t* __restrict__ em, int nwords,
                        uint32_t (*tl)[H][kSignBlock], int gl, int gbase) {
  constexpr int Wp = H * kT;
  uint32_t x[H], r2[H], op[H], r[H];
#pragma unroll
  for (int i = 0; i < H; i++) {
    x[i] = xw ? xw[gl * H + i] : 0xffffffffu;
    r2[i] = xw ? r2w[gl * H + i] : ((gl == 0 && i == 0) ? 1u : 0u);
    op[i] = em ? em[Wp + gl * H + i] : 0u;  // hi
  }
  mont_mul_ct<H>(r, op, r2, x, npx, gl, gbase);  // hi Rp mod x
  {
    uint64_t s = 0;
#pragma unroll
    for (int i = 0; i < H; i++) {
      s = (uint64_t)r[i] + (em ? em[gl * H + i] : 0u) + (s >> 32);
      r[i] = (uint32_t)s;
    }
    uint32_t tp = (uint32_t)(s >> 32);
    carry_norm_ct<H>(r, tp, gl);
    cond_sub_ct<H>(r, x, __shfl(tp, kT - 1, kT), gl, gbase);  // y < Rp, y = EM (mod x)
  }
  uint32_t base[H];
  mont_mul_ct<H>(base, r, r2, x, npx, gl, gbase);  // EM Rp mod x
#pragma unroll
  for (int i = 0; i < H; i++) op[i] = (gl == 0 && i == 0) ? 1u : 0u;
  mont_mul_ct<H>(acc, r2, op, x, npx, gl, gbase);  // Rp mod x: entry 0 and the start
#pragma unroll
  for (int i = 0; i < H; i++) {
    tl[0][i][threadIdx.x] = acc[i];
    tl[1][i][threadIdx.x] = base[i];
    r[i] = base[i];
  }
#pragma unroll 1
  for (int d = 2; d < kSignEntries; d++) {
    mont_mul_ct<H>(r, r, base, x, npx, gl, gbase);
#pragma unroll
    for (int i = 0; i < H; i++) tl[d][i][threadIdx.x] = r[i];
  }
#pragma unroll 1
  for (int t = (int)rsa::sign_windows((uint32_t)nwords) - 1; t >= 0; t--) {
    // the digit: the addresses are the loop counter's
    const uint32_t b = (uint32_t)t * rsa::kSignWin, wi = b >> 5;
    const uint64_t lo = expw ? expw[wi] : 0u, hi = (expw && wi + 1 < rsa::kHalfWords) ? expw[wi + 1] : 0u;
    const uint32_t dig = (uint32_t)(((hi << 32) | lo) >> (b & 31)) & (uint32_t)(kSignEntries - 1);
#pragma unroll 1
    for (int s = 0; s <= (int)rsa::kSignWin; s++) {
      if (s == (int)rsa::kSignWin) {  // the entry of the digit: every entry read, one kept
#pragma unroll
        for (int i = 0; i < H; i++) op[i] = 0;
#pragma unroll 4
        for (int d = 0; d < kSignEntries; d++) {
          const uint32_t hit = sign_mask(dig == (uint32_t)d);
#pragma unroll
          for (int i = 0; i < H; i++) op[i] |= tl[d][i][threadIdx.x] & hit;
        }
      } else {
#pragma unroll
        for (int i = 0; i < H; i++) op[i] = acc[i];
      }
      mont_mul_ct<H>(acc, acc, op, x, npx, gl, gbase);
    }
  }
}

// sigs[row] = the signature of the EM in words[row] (W little-endian words, from the
// prep) under the key key_id[row] names, as k big-endian bytes at the start of a
// 4 W-byte slot, the rest zero; sig_len[row] = k; status[row] = OK. A row the prep
// decided (st[row] != OK) keeps that status, a row whose fault check fails is
// SIGN_FAILED; both get a zero slot and length 0. The arrays may overlap the table's
// scratch (the add's consistency run), so none is __restrict__.
template <int W>
__global__ void __launch_bounds__(kSignBlock) rsa_sign_keyed_kernel(const uint32_t* tab, const uint32_t* key_id,
                                                                    const uint32_t* words, const uint8_t* st,
                                                                    uint64_t nrows, uint8_t* sigs, uint16_t* sig_len,
                                                                    uint8_t* status) {
  constexpr int L = W / kT, H = L / 2;
  static_assert(W % (2 * kT) == 0, "width class");
  const int gl = threadIdx.x & (kT - 1);
  const int gbase = (threadIdx.x & 63) & ~(kT - 1);
  const uint64_t row = (uint64_t)blockIdx.x * kSignGroups + threadIdx.x / kT;
  const bool inside = row < nrows;
  const uint8_t pre = inside ? st[row] : kSignSkipped;
  const uint32_t* rec = (inside && pre == kStatusOk) ? rsa_sign_record(tab, key_id[row], W) : nullptr;
  const uint32_t* em = rec ? words + row * W : nullptr;
  __shared__ uint32_t tl[kSignEntries][H][kSignBlock];
  static_assert(sizeof(tl) <= 64 * 1024, "a block's static LDS");
  // the wave's longest prime sets the number of exponent words
  uint32_t pb = rec ? rec[rsa::kSignRecPbitsWord] : 0u;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) pb = max(pb, (uint32_t)__shfl_xor((int)pb, off));
  const int nwords = (int)((__builtin_amdgcn_readfirstlane(pb) + 31) / 32);
  uint32_t m1[H], m2[H];
  sign_half_exp<H>(m1, rec ? rec + rsa::kSignRecPWord : nullptr, rec ? rec + rsa::kSignRecR2pWord : nullptr,
                   rec ? rec + rsa::kSignRecDpWord : nullptr, rec ? rec[rsa::kSignRecNppWord] : 1u, em, nwords, tl, gl,
                   gbase);
  sign_half_exp<H>(m2, rec ? rec + rsa::kSignRecQWord : nullptr, rec ? rec + rsa::kSignRecR2qWord : nullptr,
                   rec ? rec + rsa::kSignRecDqWord : nullptr, rec ? rec[rsa::kSignRecNpqWord] : 1u, em, nwords, tl, gl,
                   gbase);
  // the table held powers of EM mod p and mod q
#pragma unroll
  for (int d = 0; d < kSignEntries; d++) {
#pragma unroll
    for (int i = 0; i < H; i++) tl[d][i][threadIdx.x] = 0;
  }
  uint32_t hF[L], sF[L];
  {
    uint32_t x[H], op[H], t[H];
    const uint32_t npp = rec ? rec[rsa::kSignRecNppWord] : 1u, npq = rec ? rec[rsa::kSignRecNpqWord] : 1u;
#pragma unroll
    for (int i = 0; i < H; i++) {
      x[i] = rec ? rec[rsa::kSignRecQWord + gl * H + i] : 0xffffffffu;
      op[i] = (gl == 0 && i == 0) ? 1u : 0u;
    }
    mont_mul_ct<H>(m2, m2, op, x, npq, gl, gbase);  // plain m2 < q
#pragma unroll
    for (int i = 0; i < H; i++) {
      x[i] = rec ? rec[rsa::kSignRecPWord + gl * H + i] : 0xffffffffu;
      op[i] = rec ? rec[rsa::kSignRecR2pWord + gl * H + i] : ((gl == 0 && i == 0) ? 1u : 0u);
    }
    mont_mul_ct<H>(t, m2, op, x, npp, gl, gbase);  // m2 Rp mod p (m2 < Rp, any)
    const uint32_t neg = sub_ct<H>(m1, m1, t, gl, gbase);
    add_masked_ct<H>(m1, x, neg, gl);  // (m1 - m2) Rp mod p
#pragma unroll
    for (int i = 0; i < H; i++) op[i] = rec ? rec[rsa::kSignRecQinvWord + gl * H + i] : 0u;
    mont_mul_ct<H>(t, m1, op, x, npp, gl, gbase);  // h = qInv (m1 - m2) mod p, plain
    sign_widen<H>(hF, t, gl);
    sign_widen<H>(sF, m2, gl);
  }
  uint32_t n[L], acc[L], other[L];
  uint32_t e = 1, np = 1;
#pragma unroll
  for (int i = 0; i < L; i++) {
    n[i] = rec ? rec[rsa::kSignRecNWord + gl * L + i] : 0xffffffffu;
    other[i] = rec ? rec[rsa::kSignRecQRWord + gl * L + i] : 0u;
  }
  if (rec) {
    e = rec[rsa::kSignRecEWord];
    np = rec[rsa::kSignRecNpWord];
  }
  mont_mul_ct<L>(acc, other, hF, n, np, gl, gbase);  // q h (< n: exact)
  {
    uint64_t s = 0;  // s = m2 + q h < n
#pragma unroll
    for (int i = 0; i < L; i++) {
      s = (uint64_t)acc[i] + sF[i] + (s >> 32);
      sF[i] = (uint32_t)s;
    }
    uint32_t tp = (uint32_t)(s >> 32);
    carry_norm_ct<L>(sF, tp, gl);
  }
  // the fault check: s^e mod n by K18's chain over the unconverted base (e is public)
  uint32_t emax = e;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) emax = max(emax, (uint32_t)__shfl_xor((int)emax, off));
  const int topbit = 31 - __clz((int)__builtin_amdgcn_readfirstlane(emax));
  // s waits in the lane's own (cleared) table columns for the output: the chain carries
  // n, acc and one operand, as K18's does
#pragma unroll
  for (int i = 0; i < L; i++) {
    acc[i] = other[i] = sF[i];
    tl[i / H][i % H][threadIdx.x] = sF[i];
  }
  const int last = 2 * topbit;
  bool started = (e >> topbit) & 1u;
#pragma unroll 1
  for (int it = 0; it <= last; it++) {
    bool square = false, take = true;
    if (it < last) {
      const bool b = (e >> (topbit - 1 - (it >> 1))) & 1u;
      square = !(it & 1);
      take = started && (square || b);
      if (!square) started = started || b;
      if (!__any(take)) continue;
    } else {
#pragma unroll
      for (int i = 0; i < L; i++)
        other[i] = rec ? rec[rsa::kSignRecKWord + gl * L + i] : ((gl == 0 && i == 0) ? 1u : 0u);
    }
    uint32_t bsel[L], r[L];
#pragma unroll
    for (int i = 0; i < L; i++) bsel[i] = square ? acc[i] : other[i];
    mont_mul_ct<L>(r, acc, bsel, n, np, gl, gbase);
#pragma unroll
    for (int i = 0; i < L; i++) acc[i] = take ? r[i] : acc[i];
  }
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < L; i++) diff |= acc[i] ^ (em ? em[gl * L + i] : acc[i]);
  const bool good = rec && group_bits(__ballot(diff != 0), gbase) == 0;
#pragma unroll
  for (int i = 0; i < L; i++) {
    sF[i] = tl[i / H][i % H][threadIdx.x];
    tl[i / H][i % H][threadIdx.x] = 0;
  }
  if (!inside) return;  // every cross-lane step is behind
  const uint32_t k = good ? (rec[rsa::kSignRecBitsWord] + 7) / 8 : 0u;
  uint8_t* out = sigs + row * 4ull * W;
#pragma unroll
  for (int i = 0; i < L; i++) {
#pragma unroll
    for (int z = 0; z < 4; z++) {
      const uint32_t pos = 4u * (uint32_t)(gl * L + i) + z;  // significance; every pos < 4 W writes one byte
      if (pos < k) out[k - 1 - pos] = (uint8_t)(sF[i] >> (8 * z));
      else out[pos] = 0;
    }
  }
  if (gl == 0) {
    sig_len[row] = (uint16_t)k;
    status[row] = pre != kStatusOk ? pre : good ? kStatusOk : kSignFailed;
  }
}

template <int W>
hipError_t launch_sign_keyed(const uint32_t* tab, const uint32_t* key_id, const uint32_t* words, const uint8_t* st,
                             uint64_t n, uint8_t* sigs, uint16_t* sig_len, uint8_t* status,
                             hipStream_t s) {
  const uint64_t blocks = (n + kSignGroups - 1) / kSignGroups;
  hipLaunchKernelGGL(rsa_sign_keyed_kernel<W>, dim3((uint32_t)blocks), dim3(kSignBlock), 0, s, tab, key_id, words, st,
                     n, sigs, sig_len, status);
  return hipGetLastError();
}

hipError_t sign_keyed_any(uint32_t W, const uint32_t* tab, const uint32_t* key_id, const uint32_t* words,
                          const uint8_t* st, uint64_t n, uint8_t* sigs, uint16_t* sig_len,
                          uint8_t* status, hipStream_t s) {
  switch (W) {
    case 64: return launch_sign_keyed<64>(tab, key_id, words, st, n, sigs, sig_len, status, s);
    case 96: return launch_sign_keyed<96>(tab, key_id, words, st, n, sigs, sig_len, status, s);
    case 128: return launch_sign_keyed<128>(tab, key_id, words, st, n, sigs, sig_len, status, s);
  }
  return hipErrorInvalidValue;
}

// rows per launch of the signer: the grid's block count stays far below 2^31
constexpr uint64_t kMaxSignLaunchRows = 1ull << 22;

}  // namespace

size_t rsa_signtab_bytes() { return rsa::kSignTabBytes; }

// ws: ws_rows * rsa_ws_row_bytes(W) bytes (EM words and the prep statuses); the launches
// loop over it. sigs: 4 W-byte slots.
hipError_t launch_rsa_sign_keyed(const uint32_t* tab, const uint32_t* key_id, const uint8_t* msgs,
                                 const uint64_t* msg_off, uint32_t msg_len, const uint8_t* salts, const uint8_t* gate,
                                 uint32_t W, uint64_t n, uint8_t* sigs, uint16_t* sig_len,
                                 uint8_t* status, uint8_t* ws, uint64_t ws_rows, hipStream_t s) {
  if (W != 64 && W != 96 && W != 128) return hipErrorInvalidValue;
  ws_rows = std::min(ws_rows, kMaxSignLaunchRows);
  if (n && !ws_rows) return hipErrorInvalidValue;
  uint32_t* words = reinterpret_cast<uint32_t*>(ws);
  uint8_t* st = reinterpret_cast<uint8_t*>(words + ws_rows * W);
  for (uint64_t lo = 0; lo < n; lo += ws_rows) {
    const uint64_t m = std::min(ws_rows, n - lo);
    hipLaunchKernelGGL(rsa_sign_prep_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, s, tab, key_id + lo,
                       msg_off ? msgs : msgs + lo * msg_len, msg_off ? msg_off + lo : nullptr, msg_len,
                       salts + lo * 32, gate ? gate + lo : nullptr, W, m, words, st);
    hipError_t e = hipGetLastError();
    e = e ? e : sign_keyed_any(W, tab, key_id + lo, words, st, m, sigs + lo * 4 * W, sig_len + lo, status + lo, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// An add's consistency run over the table's scratch (rsa_sign.hpp kSignScr*): the one
// row whose key id, EM and prep status the host has put there, through the kernel
hipError_t launch_rsa_sign_selftest(uint32_t* tab, uint32_t W, hipStream_t s) {
  return sign_keyed_any(W, tab, tab + rsa::kSignScrIdWord, tab + rsa::kSignScrEmWord,
                        reinterpret_cast<const uint8_t*>(tab + rsa::kSignScrStWord), 1,
                        reinterpret_cast<uint8_t*>(tab + rsa::kSignScrSigWord),
                        reinterpret_cast<uint16_t*>(tab + rsa::kSignScrLenWord),
                        reinterpret_cast<uint8_t*>(tab + rsa::kSignScrStatusWord), s);
}
