// Ed25519 (EDDSA_ED25519_SHA512) batch verification against registered public
// keys for gfx950 -- kernel K12.
//
// Replaces, per lane, the reference's
//   Crypto.doVerify / isValid(EDDSA_ED25519_SHA512, key, sig, clear)   Crypto.kt:472-541
//   -> i2p eddsa 0.2.0 EdDSAEngine.engineVerify
// for a handful of long-lived keys (notaries, oracles, issuers) and many
// signatures. A key is registered once (ed25519_vkey_build_kernel: the i2p
// decode of A, the canonical Abyte, and the window table [d 256^j](-A),
// d = 1..128, j = 0..31, ed25519_vkey.hpp); a lane then computes the engine's
// equation literally,
//   encode([S_eff]B + [h](-A)) == R bytewise,  h = SHA-512(R || Abyte || M) mod L:
// 32 mixed additions from the table [d 256^j]B (signed 8-bit digits of S_eff), 32
// from the key's table (signed 8-bit digits of h), one inversion for the
// encoding. No doubling, no decompression, no decode of R, no lattice
// reduction, no per-lane workspace, one launch.
//
// Nothing here is secret: the gathers are indexed by the lane's own digits.
// Oracle: oracle/i2p_ed25519.py, oracle/c/ed25519.c.
#ifndef FE_QUAD
#define FE_QUAD 0
#endif
#ifndef FE_USE_ASM2
#define FE_USE_ASM2 1
#endif
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ed25519_ops.hpp"
#include "ed25519_route.hpp"
#include "ed25519_vkey.hpp"
#include "status.hpp"

namespace cordahip {

// the identity as an affine niels entry (y + x, y - x, 2dxy) = (1, 1, 0): the
// entry of a zero digit
__device__ __attribute__((aligned(64))) const uint32_t kIdentityNiels[kVkeyEntryWords] = {
    1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// ---------------------------------------------------------------------------
// Registration, once per key and device: thread g builds the entry
// [d 256^j](-A), j = g / 128, d = g % 128 + 1 -- 8 j doublings of -A, a
// double-and-add by d, one inversion -- so the 4,096 normalisations run in
// 4,096 lanes. Every group operation is the complete addition law: for a
// small-order or mixed-order key (legal in i2p 0.2.0) entries repeat or are the
// identity, and come out as such. The 32 key bytes are in the table's scratch
// words; word kVkeyOkWord answers whether they decode (ge_frombytes_i2p: y not
// range checked, x = 0 with the sign bit set accepted, no small-order check).
// A key that does not decode writes neither a table nor a record.
// slot == kVkeyBaseSlot: the table [d 256^j]B of the base point instead (once per
// device, with its first key): no key bytes, no record, no negation.
__global__ void __launch_bounds__(64) ed25519_vkey_build_kernel(uint32_t* __restrict__ vtab, uint32_t slot,
                                                                uint32_t key_id) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= kVkeyDigits * kVkeyEntries) return;
  const int j = g / kVkeyEntries, d = g % kVkeyEntries + 1;
  ge_p3 A;
  if (slot == kVkeyBaseSlot) {
    ge_base(A);
  } else {
    uint32_t w[8];
    load8(w, vtab + kVkeyKeyWord);
    const bool ok = ge_frombytes_i2p(A, w);
    if (g == 0) {
      const uint32_t flag[8] = {ok ? 1u : 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
      store8(vtab + kVkeyOkWord, flag);
    }
    if (!ok) return;
    if (g == 0) {
      // EdDSAPublicKey.Abyte = A.toByteArray(): canonical, whatever the bytes registered
      uint32_t abyte[8];
      fe_tobytes(abyte, A.Y);
      abyte[7] |= fe_isnegative(A.X) << 31;
      uint32_t* rec = vtab + kVkeyRecBase + slot * kVkeyRecWords;
      store8(rec + kVkeyRecAbyte, abyte);
      const uint32_t tail[8] = {key_id, 1u, 0u, 0u, 0u, 0u, 0u, 0u};
      store8(rec + kVkeyRecId, tail);
    }
    fe_neg(A.X, A.X);
    fe_neg(A.T, A.T);
  }
#pragma unroll 1
  for (int t = 0; t < 8 * j; t++) ge_dbl<true>(A, A);
  ge_cached pc;
  ge_to_cached(pc, A);
  ge_p3 Q;
  ge_identity(Q);
#pragma unroll 1
  for (int bit = 7; bit >= 0; bit--) {
    ge_dbl<true>(Q, Q);
    if ((d >> bit) & 1) ge_add<true>(Q, Q, pc);
  }
  store_niels_entry(vtab + (size_t)slot * kVkeyTableWords + vkey_entry_word(j, d), Q);
}

// ---------------------------------------------------------------------------
// Both scalars live in LDS, word-major, one column per thread (word w of this
// thread's scalar at col[w * 256]): a round reads a word or two of each, and
// the 16 VGPRs they would pin across the loop go to the additions.
// vkey_entry: the entry, in the table tab, of digit j of the biased scalar t
// (ed25519_vkey.hpp), and the digit's sign; a zero digit reads the identity.
CDEV const uint32_t* vkey_entry(const uint32_t* __restrict__ tab, const uint32_t* t, int j, bool& neg) {
  const int d = vkey_digit(t[(j >> 2) * 256], j);
  neg = d < 0;
  const int ad = neg ? -d : d;
  return ad ? tab + vkey_entry_word(j, ad) : kIdentityNiels;
}

#ifndef ED_VKEY_WAVES
#define ED_VKEY_WAVES 2
#endif
// the generated asm blocks (fe25519_asm.hpp) clobber the fixed accumulator
// VGPRs v160..v167, so the kernel needs a budget of >= 168 VGPRs: 512 / waves
static_assert(512 / ED_VKEY_WAVES >= 168, "fe25519_asm.hpp's v160..v167 accumulators need >= 168 VGPRs per lane");

// K12. Messages: moff / mlen non-null: lane i's message is mlen[i] bytes at
// msgs + moff[i]; else dense rows of msg_len bytes. Signatures: dense 64-byte
// rows. Statuses by precedence: UNKNOWN_KEY (the record of the id's slot holds
// another id, or none; such a lane reads nothing but that record's id and live
// words), pre[i] when non-zero (the host form's EMPTY / MALFORMED_SIG), EMPTY
// (no message byte, doVerify rules), BAD_SIG, OK. verdict word per wave by
// ballot: bit = status OK; lanes past n write nothing.
//
// The body serves two kernels. kIdx false: K12 itself, lane i is thread i. kIdx true:
// the routed instance (K14, ed25519_route.hpp): thread j below n takes lane
// i = list[j], key_id is the route array (indexed by lane), no verdict words.
template <bool kIdx>
CDEV void verify_keyed_lane(const uint32_t* __restrict__ key_id, const uint32_t* __restrict__ list,
                            const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ msgs,
                            const uint64_t* __restrict__ moff, const uint32_t* __restrict__ mlen, uint32_t msg_len,
                            uint64_t n, const uint8_t* __restrict__ pre, uint32_t empty_is_error,
                            const uint32_t* __restrict__ vtab, uint8_t* __restrict__ status,
                            unsigned long long* __restrict__ verdict) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = j < n;
  const uint64_t i = kIdx ? (active ? list[j] : 0) : j;
  __shared__ uint32_t sk[16][256];  // h and S_eff, biased: only the thread's own column is read
  uint8_t st = kStatusBadSig;
  uint32_t slot = 0;
  uint32_t len = 0;
  if (active) {
    const uint32_t id = key_id[i];
    slot = vkey_slot(id);
    len = moff ? mlen[i] : msg_len;
    const uint32_t* rec = vtab + kVkeyRecBase + slot * kVkeyRecWords;
    st = kStatusPending;
    if (!vtab || id == kVkeyNoId || rec[kVkeyRecId] != id || rec[kVkeyRecLive] != 1u) st = kVerifyUnknownKey;
    else if (pre && pre[i] != kStatusOk) st = pre[i];
    else if (len == 0 && empty_is_error) st = kStatusEmpty;  // doVerify: Crypto.kt:476 (isValid hashes it)
  }
  if (st == kStatusPending) {
    const uint32_t* rec = vtab + kVkeyRecBase + slot * kVkeyRecWords;
    const uint32_t* tab = vtab + (size_t)slot * kVkeyTableWords;
    const uint32_t* btab = vtab + (size_t)kVkeyBaseSlot * kVkeyTableWords;
    const uint8_t* msg = moff ? msgs + moff[i] : msgs + i * (uint64_t)msg_len;
    const uint32_t* t = &sk[0][threadIdx.x];
    const uint32_t* se = &sk[8][threadIdx.x];
    {
      uint32_t Rw[8], abyte[8], hd[16], h[8], S[8], tb[8], e[8], eb[8];
      load8(Rw, reinterpret_cast<const uint32_t*>(sigs + i * 64));
      load8(abyte, rec + kVkeyRecAbyte);
      sha512_segments(hd, Rw, abyte, true, msg, len);
      sc_reduce512(h, hd);
      vkey_bias(tb, h);
      load8(S, reinterpret_cast<const uint32_t*>(sigs + i * 64 + 32));
      sc_effective_S(e, S, slide_drops_carry(S));
      vkey_bias(eb, e);
#pragma unroll
      for (int q = 0; q < 8; q++) {
        sk[q][threadIdx.x] = tb[q];
        sk[8 + q][threadIdx.x] = eb[q];
      }
    }
    PHASE_BARRIER();
    // P = sum of 64 table entries, two per round: key digit r, base digit r.
    // Each gather is issued one addition ahead of its use.
    ge_p3 P;
    ge_identity(P);
    bool neg_c, neg_n;
    ge_niels cur, nxt;
    load_niels(cur, vkey_entry(tab, t, 0, neg_c), 0);
#pragma unroll 1
    for (int r = 0; r < kVkeyDigits; r++) {
      load_niels(nxt, vkey_entry(btab, se, r, neg_n), 0);
      niels_cneg(cur, neg_c);
      ge_madd<true>(P, P, cur);
      // the last round gathers digit 31 again and drops it
      load_niels(cur, vkey_entry(tab, t, min(r + 1, kVkeyDigits - 1), neg_c), 0);
      niels_cneg(nxt, neg_n);
      ge_madd<true>(P, P, nxt);
    }
    uint32_t enc[8], Rw[8];
    ge_tobytes(enc, P);
    load8(Rw, reinterpret_cast<const uint32_t*>(sigs + i * 64));  // read again: not held across the additions
    uint32_t diff = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) diff |= enc[q] ^ Rw[q];
    st = diff == 0 ? kStatusOk : kStatusBadSig;
  }
  if (active) status[i] = st;
  if (!kIdx) {
    const unsigned long long ok = __ballot(active && st == kStatusOk);
    // 256-lane blocks from lane 0: lane 0 of a wave owns a whole verdict word
    if ((threadIdx.x & 63) == 0 && active && verdict) verdict[i >> 6] = ok;
  }
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ED_VKEY_WAVES))) ed25519_verify_keyed_kernel(
    const uint32_t* __restrict__ key_id, const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ msgs,
    const uint64_t* __restrict__ moff, const uint32_t* __restrict__ mlen, uint32_t msg_len, uint64_t n,
    const uint8_t* __restrict__ pre, uint32_t empty_is_error, const uint32_t* __restrict__ vtab,
    uint8_t* __restrict__ status, unsigned long long* __restrict__ verdict) {
  verify_keyed_lane<false>(key_id, nullptr, sigs, msgs, moff, mlen, msg_len, n, pre, empty_is_error, vtab, status,
                           verdict);
}

// The routed instance: dense message rows, the lane count read from the scratch
// header; blocks past it exit at once.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ED_VKEY_WAVES)))
ed25519_verify_keyed_idx_kernel(const uint32_t* __restrict__ scratch, uint64_t lanes,
                                const uint8_t* __restrict__ sigs, const uint8_t* __restrict__ msgs, uint32_t msg_len,
                                const uint8_t* __restrict__ pre, uint32_t empty_is_error,
                                const uint32_t* __restrict__ vtab, uint8_t* __restrict__ status) {
  const uint64_t n = scratch[kRouteCntKeyed];
  if ((uint64_t)blockIdx.x * blockDim.x >= n) return;
  verify_keyed_lane<true>(scratch + route_off_route(lanes), scratch + route_off_keyed(lanes), sigs, msgs, nullptr,
                          nullptr, msg_len, n, pre, empty_is_error, vtab, status, nullptr);
}

// ---------------------------------------------------------------------------
// host-side launchers (called by cordahip.cpp)
size_t ed25519_vkey_bytes() { return (size_t)kVkeyAllWords * sizeof(uint32_t); }

hipError_t launch_ed25519_vkey_build(uint32_t* vtab, uint32_t key_id, hipStream_t s) {
  hipLaunchKernelGGL(ed25519_vkey_build_kernel, dim3(kVkeyDigits * kVkeyEntries / 64), dim3(64), 0, s, vtab,
                     vkey_slot(key_id), key_id);
  return hipGetLastError();
}

hipError_t launch_ed25519_vkey_base(uint32_t* vtab, hipStream_t s) {
  hipLaunchKernelGGL(ed25519_vkey_build_kernel, dim3(kVkeyDigits * kVkeyEntries / 64), dim3(64), 0, s, vtab,
                     kVkeyBaseSlot, 0u);
  return hipGetLastError();
}

hipError_t launch_ed25519_verify_keyed(const uint32_t* key_id, const uint8_t* sigs, const uint8_t* msgs,
                                       const uint64_t* moff, const uint32_t* mlen, uint32_t msg_len, uint64_t n,
                                       const uint8_t* pre, uint32_t flags, const uint32_t* vtab, uint8_t* status,
                                       unsigned long long* verdict, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ed25519_verify_keyed_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, key_id, sigs, msgs, moff,
                     mlen, msg_len, n, pre, (flags & 1u) ? 0u : 1u, vtab, status, verdict);
  return hipGetLastError();
}

// K12 over the keyed list of a routed batch of `lanes` lanes (scratch:
// ed25519_route.hpp): the grid covers every lane, the kernel reads the count
hipError_t launch_ed25519_verify_keyed_idx(const uint32_t* scratch, uint64_t lanes, const uint8_t* sigs,
                                           const uint8_t* msgs, uint32_t msg_len, const uint8_t* pre, uint32_t flags,
                                           const uint32_t* vtab, uint8_t* status, hipStream_t s) {
  if (lanes == 0) return hipSuccess;
  const uint64_t blocks = (lanes + 255) / 256;
  if (blocks > 0x7fffffffull || !vtab) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ed25519_verify_keyed_idx_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, scratch, lanes, sigs,
                     msgs, msg_len, pre, (flags & 1u) ? 0u : 1u, vtab, status);
  return hipGetLastError();
}

}  // namespace cordahip
