// Ed25519 verification ladder for gfx950 — second kernel of K1.
//
// Per lane (record written by ed25519_prep_half_kernel, ed25519.hip): decide
//   [e]B + [c0](+-A) + [c1](-R) == O
// with |c0|, c1 ~ 2^128 (c0 == c1 h mod 8L, c1 odd) and e = c1 S_eff mod L: the
// i2p 0.2.0 cofactorless check encode([S]B - [h]A) == R rewritten over
// half-size scalars (T. Pornin, ePrint 2020/454; the equivalence argument is in
// ed25519.hip above half_scalars). 2-bit Booth windows over both scalars at
// once: one addition per window of an entry i(-A) + j(-R) of the per-lane joint
// table (ed25519_joint.hpp; gathered from the workspace one window ahead, so
// the two doublings hide the load; which entry, and the fixed-base digits, come
// recoded from the prep: ed25519_sel.hpp), kBBits-bit Booth windows over B and
// B' = [2^(kBDigitsLo kBBits)]B from shared tables (ed25519_ws.hpp). Digit
// positions are the same in every lane, so the ladder never diverges. Three
// group operations are cut to what the verdict needs: the top window's entry
// is loaded as the accumulator instead of added to the identity
// (ED_LADDER_TOP_LOAD), the high half of e has one digit fewer than the low
// half at 20 and 18 bits, and the last addition stops at E, F, H
// (ED_LADDER_LAST_EH, ge25519.hpp ge_madd_is_identity; no inversion either way).
// A wave runs the windows of its longest lane, so a block hands its lanes to its
// four waves in window-count order (ED_LADDER_ORDER); verdict words by ballot,
// by the block's last wave.
// field products in hand-scheduled pairs (ge25519.hpp fe_mul_pair, fe25519_asm.hpp)
#ifndef FE_USE_ASM2
#define FE_USE_ASM2 1
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ed25519_route.hpp"
#include "ed25519_ws.hpp"
#include "status.hpp"

namespace cordahip {

// the identity entry: behind the B tables (ED_IDENT_GLOBAL, ed25519_ws.hpp) or
// this constant, whose generic address turns the entry gather into flat loads
__device__ __attribute__((aligned(64))) const uint32_t kIdentityCached[kWhEntryWords] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0,   // Y + X
                                                            1, 0, 0, 0, 0, 0, 0, 0, 0, 0,   // Y - X
                                                            1, 0, 0, 0, 0, 0, 0, 0, 0, 0,   // Z
                                                            0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // 2dT

// waves per SIMD the register allocation targets (2: up to 256 VGPRs)
#ifndef ED_LADDER_WAVES
#define ED_LADDER_WAVES 2
#endif
// the generated asm blocks (fe25519_asm.hpp) clobber the fixed accumulator
// VGPRs v160..v167, so the kernel needs a budget of >= 168 VGPRs: 512 / waves
static_assert(512 / ED_LADDER_WAVES >= 168, "fe25519_asm.hpp's v160..v167 accumulators need >= 168 VGPRs per lane");

// ED_LADDER_ORDER: a block's lanes go to its four waves in window-count order
// (ladder_half_lane). Keys of the counting rank: counts kOrderLo .. kOrderHi,
// then the lanes past the batch.
#ifndef ED_LADDER_ORDER
#define ED_LADDER_ORDER 1
#endif
#if ED_LADDER_ORDER && !ED_SEL_STREAM
#error "ED_LADDER_ORDER ranks the lanes by the selector stream's window count"
#endif
// ED_LADDER_TOP_LOAD: the top window sets P from its entry (ge_from_cached)
// instead of adding the entry to the identity; 0: the addition.
// ED_LADDER_LAST_EH: the verdict comes from the last addition's E, F, H
// without its output stage; 0: from X, Y, Z of the full addition.
#ifndef ED_LADDER_TOP_LOAD
#define ED_LADDER_TOP_LOAD 1
#endif
#ifndef ED_LADDER_LAST_EH
#define ED_LADDER_LAST_EH 1
#endif
static constexpr int kOrderLo = 60, kOrderHi = 74, kOrderKeys = kOrderHi - kOrderLo + 2;
static_assert(kOrderKeys <= 64, "one lane of a wave per key");

// The body serves two kernels. kIdx false: the ladder itself, record li is lane
// base + li. kIdx true: the routed instance (K14, ed25519_route.hpp): record li is
// lane list[base + li], no verdict words.
template <bool kIdx>
CDEV void ladder_half_lane(uint64_t base, uint64_t m, const uint32_t* __restrict__ btab,
                           const uint32_t* __restrict__ ws, uint8_t* __restrict__ status,
                           unsigned long long* __restrict__ verdict, const uint32_t* __restrict__ list) {
  const uint64_t blk = (uint64_t)blockIdx.x * blockDim.x;
#if ED_LADDER_ORDER
  // This thread loads the selector words of record blk + threadIdx.x, the block
  // ranks its 256 records by window count, and thread t then runs the record of
  // rank t: each wave's W = its longest lane, so the block's waves get its
  // lanes in count order and only the last one pays for the block's longest.
  __shared__ uint32_t sk[kSelWords][256];
  __shared__ uint8_t order_src[256];               // rank -> thread that loaded the record
  __shared__ uint32_t order_cnt[4][kOrderKeys];    // per wave: lanes of each key
  __shared__ uint32_t order_done;                  // waves that have left their ok bits (verdict words below)
  uint64_t li;
  {
    const uint64_t l0 = blk + threadIdx.x;
    const uint32_t* r0 = ws + (l0 < m ? l0 : m - 1) * kWhLaneWords;
    const uint4* r4 = reinterpret_cast<const uint4*>(r0 + kWhSel);
    uint4 v[(kSelWords + 3) / 4];
#pragma unroll
    for (int q = 0; q < (kSelWords + 3) / 4; q++) v[q] = r4[q];
    static_assert(kSelMeta / 4 == 7 && (kSelWords + 3) / 4 == 8, "the count is in the last quad");
    const uint32_t meta = kSelMeta % 4 == 2 ? v[7].z : v[7].w;
    static_assert(kSelMeta % 4 >= 2, "its third or fourth word");
    // a stable counting rank over the keys: the window count clamped to
    // [kOrderLo, kOrderHi] (fewer or more are rare and only order less well),
    // lanes past the batch last: they lengthen no wave (W below skips them)
    const int cnt = (int)(meta >> 16);
    const int key = l0 < m ? min(max(cnt, kOrderLo), kOrderHi) - kOrderLo : kOrderKeys - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t before = 0, mine = 0;
#pragma unroll
    for (int k = 0; k < kOrderKeys; k++) {
      const unsigned long long mk = __ballot(key == k);
      if (key == k) before = (uint32_t)__popcll(mk & ((1ull << lane) - 1));
      if (lane == k) mine = (uint32_t)__popcll(mk);
    }
    if (lane < kOrderKeys) order_cnt[wave][lane] = mine;
    if (threadIdx.x == 0) order_done = 0;
    __syncthreads();
    uint32_t rank = before;
#pragma unroll
    for (int k = 0; k < kOrderKeys; k++)
#pragma unroll
      for (int w = 0; w < 4; w++) {
        const uint32_t c = order_cnt[w][k];
        rank += (k < key || (k == key && w < wave)) ? c : 0u;
      }
    order_src[rank] = (uint8_t)threadIdx.x;
#pragma unroll
    for (int q = 0; q < (kSelWords + 3) / 4; q++) {
      const uint32_t w[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
      for (int t = 0; t < 4; t++)
        if (4 * q + t < kSelWords) sk[4 * q + t][rank] = w[t];
    }
    __syncthreads();
    li = blk + order_src[threadIdx.x];
  }
#else
  const uint64_t li = blk + threadIdx.x;
#endif
  const bool active = li < m;
  const uint64_t lc = active ? li : m - 1;  // inactive lanes replay the last record, discard it
  const uint32_t* rec = ws + lc * kWhLaneWords;
#if ED_IDENT_GLOBAL
  const uint32_t* ident = btab + kBIdentityWord;  // a global pointer like rec: the gather stays global_load
#else
  const uint32_t* ident = kIdentityCached;
#endif
  const uint32_t* btab2 = btab + kBTableEntries * kBEntryWords;
  ge_p3 P;
  ge_identity(P);
#if ED_SEL_STREAM
  // the selector stream (ed25519_sel.hpp) lives in LDS, word-major, one column
  // per thread: a window reads one word of it, a fixed-base window three more,
  // and no VGPR is pinned across the loop
#if !ED_LADDER_ORDER
  __shared__ uint32_t sk[kSelWords][256];
  {
    const uint4* r4 = reinterpret_cast<const uint4*>(rec + kWhSel);
#pragma unroll
    for (int q = 0; q < (kSelWords + 3) / 4; q++) {
      const uint4 v = r4[q];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int t = 0; t < 4; t++)
        if (4 * q + t < kSelWords) sk[4 * q + t][threadIdx.x] = w[t];
    }
  }
#endif
  const uint32_t* col = &sk[0][threadIdx.x];
  // at least the windows the fixed-base digits need (kBDigitsLo digits of
  // kBBits bits over B: kBMinWindows); |c0|, c1 ~ 2^128 give 65. Lanes with
  // fewer windows of their own select the identity above them. (A count is at
  // most 129.)
#if ED_LADDER_ORDER
  const int own = active ? (int)(col[kSelMeta * 256] >> 16) : 0;  // a lane past the batch follows its wave
#else
  const int own = (int)(col[kSelMeta * 256] >> 16);
#endif
  const int W = min(max(wave_max(own), kBMinWindows), kSelWindows);
  bool zero = false;
  // window j's selector is read while window j + 1 computes; its word and
  // field are the same in every lane
  uint32_t selw = col[((W - 1) / kSelPerWord) * 256];
  for (int j = W - 1; j >= 0; j--) {
    const int jn = max(j - 1, 0);
    const uint32_t selw_next = col[(jn / kSelPerWord) * 256];
    const uint32_t sel = selw >> (kSelBits * (j % kSelPerWord));
    const uint32_t idx = sel & 15u;
    const bool neg = sel & kSelNeg;
    ge_cached c;  // issued before the doublings, consumed after them
    load_cached(c, idx == kSelIdentity ? ident : rec + kWhTab + idx * kWhEntryWords);
    // fixed-base window (W is the wave's maximum and may exceed 65: the low
    // digits' windows end at digit kBDigitsLo - 1, the high digits ride on B';
    // the windows from kBDigitsHi up have a low digit only): its digits are
    // read here, ahead of the doublings
    const bool bwin = j % kBWin == 0 && j < kBDigitsLo * kBWin;
    const int t = j / kBWin;
    const bool hi = t < kBDigitsHi;
    uint32_t m0 = 0, m1 = 0, sg = 0;
    if (bwin) {
      m0 = sel_bmag(col, 256, t);
      if (hi) m1 = sel_bmag(col, 256, t + kBDigitsLo);
      sg = col[kSelMeta * 256];
    }
    const bool top = j == W - 1;
    if (!top) {
      ge_dbl<false>(P, P);
      ge_dbl<true>(P, P);
    }
    cached_cneg(c, neg);
    if (bwin) {
      // the gather of each niels entry is issued one addition ahead of its use
      // (registers allow no more). The low digit's addition comes last, so the
      // windows without a high digit skip the middle one and share the rest.
      ge_niels nb;
      uint32_t pad[2];
      bool nbneg = sel_bneg(sg, hi ? t + kBDigitsLo : t);
      load_niels(nb, hi ? btab2 : btab, (int)(hi ? m1 : m0), pad);
      ge_add<true>(P, P, c);  // the top window too: it is one only in a wave without scalars of its own
      if (hi) {
        ge_niels nb0;
        uint32_t pad0[2];
        load_niels(nb0, btab, (int)m0, pad0);
        niels_pad_use(pad);
        niels_cneg(nb, nbneg);
        ge_madd<true>(P, P, nb);
        nb = nb0;
        pad[0] = pad0[0];
        pad[1] = pad0[1];
        nbneg = sel_bneg(sg, t);
      }
      niels_pad_use(pad);
      niels_cneg(nb, nbneg);
#if ED_LADDER_LAST_EH
      if (j == 0) zero = ge_madd_is_identity(P, nb);
      else ge_madd<false>(P, P, nb);
#else
      ge_madd<false>(P, P, nb);
#endif
    } else if (ED_LADDER_TOP_LOAD && top) {
      ge_from_cached(P, c);  // the two doublings that follow need no T
    } else {
      ge_add<false>(P, P, c);
    }
    selw = selw_next;
  }
#else
  static_assert(kBBits == 16 && kBDigitsLo == kBDigitsHi, "without the selector stream the ladder is 16-bit only");
  // |c0|, c1 and e live in LDS (word-major, one column per thread): each window
  // reads two words of each, and the 24 VGPRs they would pin across the loop
  // go to the group formulas' wider product blocks instead
  __shared__ uint32_t sk[24][256];
  const uint32_t* ska = &sk[0][threadIdx.x];
  const uint32_t* skr = &sk[8][threadIdx.x];
  const uint32_t* ske = &sk[16][threadIdx.x];
  int bits;
  {
    uint32_t ka[8], kr[8], e[8];
    load8(ka, rec + kWhKa);
    load8(kr, rec + kWhKr);
    load8(e, rec + kWhE);
#pragma unroll
    for (int q = 0; q < 8; q++) {
      sk[q][threadIdx.x] = ka[q];
      sk[8 + q][threadIdx.x] = kr[q];
      sk[16 + q][threadIdx.x] = e[q];
    }
    bits = max(mp8_bitlen(ka), mp8_bitlen(kr));
  }
  const bool c0neg = rec[kWhFlags] & 1u;  // [c0](-A) with c0 < 0 is [|c0|]A: flip the digit signs
  // at least the windows the fixed-base digits need (e's low half: kBDigitsLo
  // digits of kBBits bits); |c0|, c1 ~ 2^128 give 65
  const int W = max(wave_max((bits + 2) / 2), kBMinWindows);
  for (int j = W - 1; j >= 0; j--) {
    const joint_sel sel = joint_select(joint_booth2(ska, 256, 8, j), joint_booth2(skr, 256, 8, j), c0neg);
    ge_cached c;  // issued before the doublings, consumed after them
    load_cached(c, table_entry(rec, sel.idx, ident));
    if (j != W - 1) {
      ge_dbl<false>(P, P);
      ge_dbl<true>(P, P);
    }
    cached_cneg(c, sel.neg);
    // fixed-base window: the L2 gather of each niels entry is issued one
    // addition ahead of its use (registers allow no more)
    // (W is the wave's maximum and may exceed 65: the low half's windows end at
    // digit kBDigitsLo - 1, the high half's digits ride on B')
    const bool bwin = j % (kBBits / 2) == 0 && j < kBDigitsLo * (kBBits / 2);
    if (bwin) {
      const int d0 = booth_digit_col<kBBits>(ske, j / (kBBits / 2));
      const int d1 = booth_digit_col<kBBits>(ske, j / (kBBits / 2) + kBDigitsLo);
      ge_niels nb0, nb1;
      load_niels(nb0, btab, d0 < 0 ? -d0 : d0);
      ge_add<true>(P, P, c);
      load_niels(nb1, btab2, d1 < 0 ? -d1 : d1);
      niels_cneg(nb0, d0 < 0);
      ge_madd<true>(P, P, nb0);
      niels_cneg(nb1, d1 < 0);
      ge_madd<false>(P, P, nb1);
    } else {
      ge_add<false>(P, P, c);
    }
  }
  fe d;
  fe_sub(d, P.Y, P.Z);
  const bool zero = fe_iszero(P.X) && fe_iszero(d);
#endif
#if ED_SEL_STREAM && !ED_LADDER_LAST_EH
  {
    fe d;
    fe_sub(d, P.Y, P.Z);
    zero = fe_iszero(P.X) && fe_iszero(d);  // P == O is X == 0 and Y == Z
  }
#endif
  const uint64_t i = kIdx ? (active ? list[base + li] : 0) : base + li;
  uint8_t st = kStatusBadSig;
  if (active) {
    st = status[i];
    if (st == kStatusPending) {
      st = zero ? kStatusOk : kStatusBadSig;
      status[i] = st;
    }
  }
  if (!kIdx) {
#if ED_LADDER_ORDER
    // Verdict words are in lane order and a wave's lanes are not: every wave
    // leaves its ok bits in LDS under the threads that loaded the records, and
    // the wave that finishes last turns them into the block's four words. No
    // barrier: a finished wave gives its registers back at once.
    __shared__ uint8_t order_ok[256];
    order_ok[li - blk] = active && st == kStatusOk;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    uint32_t arrived = 0;
    if ((threadIdx.x & 63) == 0)
      arrived = __hip_atomic_fetch_add(&order_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    arrived = (uint32_t)__shfl((int)arrived, 0);
    if (arrived == blockDim.x / 64 - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      const int lane = threadIdx.x & 63;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const unsigned long long ok = __ballot(order_ok[64 * q + lane] != 0);
        // base is a multiple of 64 (workspace chunks are), and so is blk: word q is the block's own
        if (lane == q && blk + 64 * q < m && verdict) verdict[(base + blk + 64 * q) >> 6] = ok;
      }
    }
#else
    const unsigned long long ok = __ballot(active && st == kStatusOk);
    // base is a multiple of 64 (workspace chunks are), so lane 0 of a wave owns a whole verdict word
    if ((threadIdx.x & 63) == 0 && active && verdict) verdict[i >> 6] = ok;
#endif
  }
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ED_LADDER_WAVES))) ed25519_ladder_half_kernel(
    uint64_t base, uint64_t m, const uint32_t* __restrict__ btab, const uint32_t* __restrict__ ws,
    uint8_t* __restrict__ status, unsigned long long* __restrict__ verdict) {
  ladder_half_lane<false>(base, m, btab, ws, status, verdict, nullptr);
}

// The routed instance: the workspace chunk at list position base holds
// route_chunk_lanes(generic count, base, m) records; a chunk or a block wholly past
// the count does nothing.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ED_LADDER_WAVES)))
ed25519_ladder_half_idx_kernel(uint64_t base, uint64_t m, const uint32_t* __restrict__ btab,
                               const uint32_t* __restrict__ ws, uint8_t* __restrict__ status,
                               const uint32_t* __restrict__ scratch, uint64_t lanes) {
  const uint64_t mm = route_chunk_lanes(scratch[kRouteCntGeneric], base, m);
  if ((uint64_t)blockIdx.x * blockDim.x >= mm) return;
  ladder_half_lane<true>(base, mm, btab, ws, status, nullptr, scratch + route_off_generic(lanes));
}

hipError_t launch_ed25519_ladder(uint64_t base, uint64_t m, const uint32_t* btab, const uint32_t* ws, uint8_t* status,
                                 unsigned long long* verdict, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((m + 255) / 256);
  hipLaunchKernelGGL(ed25519_ladder_half_kernel, dim3(blocks), dim3(256), 0, s, base, m, btab, ws, status, verdict);
  return hipGetLastError();
}

hipError_t launch_ed25519_ladder_idx(uint64_t base, uint64_t m, const uint32_t* btab, const uint32_t* ws,
                                     uint8_t* status, const uint32_t* scratch, uint64_t lanes, hipStream_t s) {
  const uint32_t blocks = (uint32_t)((m + 255) / 256);
  hipLaunchKernelGGL(ed25519_ladder_half_idx_kernel, dim3(blocks), dim3(256), 0, s, base, m, btab, ws, status, scratch,
                     lanes);
  return hipGetLastError();
}

}  // namespace cordahip
