// Per-lane classification and row packing of generic signature batches
// (cordahip_sig_batch, the Crypto.isValid / doVerify batch of Crypto.kt:472-541):
// the host side of host_batch.cpp's pipelines, in a header of its own so that
// tools/pack_bench.cpp measures exactly this code on the CPU (the host budget
// of one process driving several GPUs). No HIP here. Every decision about a
// lane -- its class, a direct status, a row's pre-status -- is sig_pack.hpp's, the rule
// the GPU packer (K23) runs too: one rule, not two.
//
// MV is the message view (runtime.hpp MsgView): len(i), ptr(i).
#pragma once
#include <stdint.h>

#include <cstring>

#include "../../include/cordahip.h"
#include "der.hpp"
#include "rsa_key.hpp"
#include "sig_pack.hpp"

namespace cordahip {
namespace rt {

// ---- the two sources of Ed25519 rows --------------------------------------------
// Ed25519 row of lane i of a cordahip_sig_batch (message length L): the
// Crypto.doVerify require()s and the engine's length check as the pre-status
template <class MV>
inline void pack_ed_row(const cordahip_sig_batch* b, const MV& mv, bool do_verify, uint64_t i, uint32_t L,
                        uint8_t* key, uint8_t* sig, uint8_t* msg, uint8_t* pre) {
  std::memcpy(key, b->key + b->key_off[i], 32);
  const uint64_t sl = b->sig_off[i + 1] - b->sig_off[i];
  const uint8_t st = sigpack::ed_pre(do_verify, sl, L);  // Crypto.kt:475-476, then EdDSAEngine: signature length
  if (st == CORDAHIP_STATUS_OK) std::memcpy(sig, b->sig + b->sig_off[i], 64);
  else std::memset(sig, 0, 64);
  *pre = st;
  if (!msg) return;  // device-side message (MsgView::dev): gathered on the GPU
  if (L == 32) std::memcpy(msg, mv.ptr(i), 32);
  else if (L) std::memcpy(msg, mv.ptr(i), L);
}

// Lane classes of a generic batch: the per-lane checks that precede the
// engines (statuses decided here are written at once). kBadCsr: the lane's CSR
// ranges are not inside the batch's buffers (csr_check.hpp: the batch fails with
// CORDAHIP_ERR_INVALID_ARG before its chunk is packed).
// kRsa: an RSA_SHA256 lane the GPU verifies (CORDAHIP_FLAG_RSA_ON_DEVICE): not a row
// of the chunk, its status comes from the batch's RSA section (host_batch.cpp).
// kRsaBase + c: such a lane of width class c (0, 1, 2: 64, 96, 128 words) where it is a
// row of its chunk's RSA section (rsa_in_chunks; classify's rsa_class says which).
enum : uint16_t { kDirect = 0, kEc = 1, kEdBase = 2, kRsaBase = 0xfff0, kRsa = 0xfffe, kBadCsr = 0xffff };

// the lane's ranges, before any byte of it is read: non-decreasing and inside
// the declared buffers (key_off[i + 1] <= key_bytes, ...; messages of a signed-tx
// batch are its transactions' ids, checked with the transactions)
template <class MV>
inline bool lane_ranges_ok(const cordahip_sig_batch* b, const MV& mv, uint64_t i) {
  const uint64_t k0 = b->key_off[i], k1 = b->key_off[i + 1], s0 = b->sig_off[i], s1 = b->sig_off[i + 1];
  if (!sigpack::ranges_ok(k0, k1, b->key_bytes, s0, s1, b->sig_bytes)) return false;
  return mv.tx_of || (mv.off[i + 1] >= mv.off[i] && mv.off[i + 1] <= b->msg_bytes);
}

// does the batch send its RSA_SHA256 lanes to the GPU? A generic batch says so in its
// flags; the signed-tx calls, whose structs carry no flags, set the same bit in the
// batch they hand to the pipeline while cordahip_set_rsa_on_device is on.
template <class MV>
inline bool rsa_on_device(const cordahip_sig_batch* b, const MV&) {
  return (b->flags & CORDAHIP_FLAG_RSA_ON_DEVICE) != 0;
}
// ... as a third section of each chunk (signed-tx batches: the messages are ids in HBM,
// known chunk by chunk) instead of a section of the whole shard beside the chunks
template <class MV>
inline bool rsa_in_chunks(const cordahip_sig_batch* b, const MV& mv) {
  return (b->flags & CORDAHIP_FLAG_RSA_ON_DEVICE) && mv.tx_of;
}

// What the host decides of RSA lane i (ranges checked): BAD_KEY / UNSUPPORTED from
// the key (rsa_key.hpp parse_public_key), then EMPTY under doVerify rules, then
// BAD_SIG for a signature longer than the modulus (PSSSigner: false); kRsaToDevice
// with pk filled for the lanes whose verdict needs the arithmetic.
constexpr uint8_t kRsaToDevice = sigpack::kRsaToDevice;
template <class MV>
inline uint8_t rsa_lane_pre(const cordahip_sig_batch* b, const MV& mv, bool do_verify, uint64_t i,
                            rsa::PublicKey& pk) {
  rsa::KeyView kv;
  const uint8_t st = sigpack::rsa_pre(b->key + b->key_off[i], b->key_off[i + 1] - b->key_off[i],
                                      b->sig_off[i + 1] - b->sig_off[i], mv.len(i), do_verify, kv);
  if (st == kRsaToDevice) rsa::key_of_view(kv, pk);  // the modulus materialised, for pack_rsa_row
  return st;
}

// RSA row r of a class-W stage: the modulus padded to W words, e, the signature
// right as it came (big-endian, at most 4 W bytes) and its length
inline void pack_rsa_row(const cordahip_sig_batch* b, uint64_t i, const rsa::PublicKey& pk, uint32_t W, uint64_t r,
                         uint32_t* hmod, uint32_t* hexp, uint8_t* hsig, uint16_t* hsl) {
  std::memcpy(hmod + r * W, pk.n, 4ull * W);
  hexp[r] = pk.e;
  const uint64_t sl = b->sig_off[i + 1] - b->sig_off[i];  // <= ceil(bits / 8) <= 4 W (rsa_lane_pre)
  std::memcpy(hsig + r * 4ull * W, b->sig + b->sig_off[i], sl);
  std::memset(hsig + r * 4ull * W + sl, 0, 4ull * W - sl);
  hsl[r] = (uint16_t)sl;
}

template <class MV>
inline uint16_t classify(const cordahip_sig_batch* b, const MV& mv, uint64_t i, uint64_t& mlen,
                         uint32_t* rsa_class = nullptr) {
  mlen = 0;
  if (!lane_ranges_ok(b, mv, i)) return kBadCsr;
  const uint64_t k0 = b->key_off[i], k1 = b->key_off[i + 1];
  mlen = mv.len(i);
  rsa::KeyView kv;
  const sigpack::Lane l =
      sigpack::lane_rule(b->scheme[i], b->key + k0, k1 - k0, b->sig_off[i + 1] - b->sig_off[i], mlen,
                         !(b->flags & CORDAHIP_FLAG_IS_VALID), rsa_on_device(b, mv), kv);
  if (l.cls == sigpack::kEd) return kEdBase;  // + the piece-local message-length group
  if (l.cls == sigpack::kEc) return kEc;
  if (l.cls == sigpack::kDirect) {
    b->status[i] = l.status;
    return kDirect;
  }
  if (rsa_class) *rsa_class = l.cls - sigpack::kRsa0;
  return kRsa;
}

// ECDSA slot packing of lane i into row r (messages CSR at *mo)
template <class MV>
inline void pack_ec_row(const cordahip_sig_batch* b, const MV& mv, bool do_verify, uint64_t i, uint64_t r, uint8_t* hsc, uint8_t* hk,
                        uint8_t* hkl, uint8_t* hs, uint8_t* hsl, uint8_t* hm, uint64_t* hmo, uint8_t* hp,
                        uint64_t& mo, uint32_t* hidx, uint64_t t0 = 0) {
  hsc[r] = b->scheme[i];
  const uint64_t kl = b->key_off[i + 1] - b->key_off[i];  // 33 or 65 (classified)
  std::memcpy(hk + r * 65, b->key + b->key_off[i], kl);
  std::memset(hk + r * 65 + kl, 0, 65 - kl);
  hkl[r] = (uint8_t)kl;
  const uint64_t sl = b->sig_off[i + 1] - b->sig_off[i];
  const uint64_t ml = mv.len(i);
  uint8_t pre = CORDAHIP_STATUS_OK;
  if (sl <= 72) {
    std::memcpy(hs + r * 72, b->sig + b->sig_off[i], sl);
    std::memset(hs + r * 72 + sl, 0, 72 - sl);
    hsl[r] = (uint8_t)sl;
  } else {
    // longer than the slot: no r, s < n fits, so the DER rules alone decide (BC:
    // well-formed -> false, else SignatureException); the kernel still decodes
    // the key first, so key errors keep precedence
    pre = sigpack::ec_pre(do_verify, b->sig + b->sig_off[i], sl, ml);
    std::memset(hs + r * 72, 0, 72);
    hsl[r] = 72;
  }
  hp[r] = pre;
  hmo[r] = mo;
  if (hidx) hidx[r] = (uint32_t)(mv.tx_of[i] - t0);  // the row is gathered on the device
  else std::memcpy(hm + mo, mv.ptr(i), ml);
  mo += ml;
}

// ---- cordahip_sign chunks (a batch that passed check_sign_batch) ----------------
// Lanes [a, a + m) go to the device as dense 32-byte rows when every message of
// the chunk has 32 bytes (transaction ids: the signer's one-block shape), else
// each message at a 16-byte-aligned offset of the stage with its length beside it.
struct SignLayout {
  bool dense;
  uint64_t bytes;  // message bytes of the stage
};
// poff[m]: the lanes' offsets in the stage (written only for a chunk that is not dense)
// msg_off: the batch's message offsets (cordahip_verify_keyed chunks share the layout)
inline SignLayout msg_chunk_layout(const uint64_t* msg_off, uint64_t a, uint64_t m, uint64_t* poff) {
  SignLayout l{true, m * 32};
  for (uint64_t i = 0; i < m && l.dense; i++) l.dense = msg_off[a + i + 1] - msg_off[a + i] == 32;
  if (l.dense) return l;
  l.bytes = 0;
  for (uint64_t i = 0; i < m; i++) {
    poff[i] = l.bytes;
    l.bytes += (msg_off[a + i + 1] - msg_off[a + i] + 15) / 16 * 16;
  }
  return l;
}
inline SignLayout sign_chunk_layout(const cordahip_sign_batch* b, uint64_t a, uint64_t m, uint64_t* poff) {
  return msg_chunk_layout(b->msg_off, a, m, poff);
}
// the message half of row i: the len bytes at msg + o to the row's place in the stage and
// -- not dense -- that place and the length beside them
inline void pack_msg(const uint8_t* msg, uint64_t o, uint64_t len, uint64_t i, const SignLayout& l, const uint64_t* poff,
                     uint8_t* hm, uint64_t* ho, uint32_t* hl) {
  const uint64_t p = l.dense ? i * 32 : poff[i];
  if (len) std::memcpy(hm + p, msg + o, len);
  if (!l.dense) {
    ho[i] = p;
    hl[i] = (uint32_t)len;
  }
}
// rows [x, y) of the chunk at lane a: key ids, gate bytes (b->gate != NULL), messages, and
// -- not dense -- offsets and lengths. B: cordahip_sign_batch or cordahip_ecdsa_sign_batch.
template <class B>
inline void sign_pack_rows(const B* b, uint64_t a, uint64_t x, uint64_t y, const SignLayout& l,
                           const uint64_t* poff, uint32_t* hid, uint8_t* hgate, uint8_t* hm, uint64_t* ho,
                           uint32_t* hl) {
  for (uint64_t i = x; i < y; i++) {
    const uint64_t o = b->msg_off[a + i], len = b->msg_off[a + i + 1] - o;
    hid[i] = b->key_id[a + i];
    if (b->gate) hgate[i] = b->gate[a + i];
    pack_msg(b->msg, o, len, i, l, poff, hm, ho, hl);
  }
}

// ---- cordahip_verify_keyed chunks (a batch that passed check_keyed_sig_batch) ----
// Messages as in a signing chunk (msg_chunk_layout). Rows [x, y) of the chunk at lane
// a: key ids, the 64-byte signature rows with the statuses the host decides as in
// pack_ed_row -- the Crypto.doVerify require()s, then the engine's length check; such
// a lane gets a zero row -- messages, and -- not dense -- offsets and lengths
inline void keyed_pack_rows(const cordahip_keyed_sig_batch* b, uint64_t a, uint64_t x, uint64_t y, const SignLayout& l,
                            const uint64_t* poff, uint32_t* hid, uint8_t* hsig, uint8_t* hpre, uint8_t* hm,
                            uint64_t* ho, uint32_t* hl) {
  const bool do_verify = !(b->flags & CORDAHIP_FLAG_IS_VALID);
  for (uint64_t i = x; i < y; i++) {
    const uint64_t o = b->msg_off[a + i], len = b->msg_off[a + i + 1] - o;
    const uint64_t so = b->sig_off[a + i], sl = b->sig_off[a + i + 1] - so;
    hid[i] = b->key_id[a + i];
    uint8_t st = CORDAHIP_STATUS_OK;
    if (do_verify && (sl == 0 || len == 0)) st = CORDAHIP_STATUS_EMPTY;  // Crypto.kt:475-476
    else if (sl != 64) st = CORDAHIP_STATUS_MALFORMED_SIG;               // EdDSAEngine: signature length
    if (st == CORDAHIP_STATUS_OK) std::memcpy(hsig + i * 64, b->sig + so, 64);
    else std::memset(hsig + i * 64, 0, 64);
    hpre[i] = st;
    pack_msg(b->msg, o, len, i, l, poff, hm, ho, hl);
  }
}

// ---- cordahip_ecdsa_verify_keyed chunks (a batch that passed check_keyed_sig_batch) ----
// As keyed_pack_rows, with the DER signatures in 72-byte slots and their lengths
// beside them. A signature longer than its slot holds no r, s < n, so the DER rules
// alone decide it here, as in pack_ec_row: EMPTY first for an empty message under
// doVerify, else well-formed -> BAD_SIG, else MALFORMED_SIG; such a lane gets a zero
// slot of length 72. Every other decision is the kernel's (hpre stays OK).
inline void keyed_ec_pack_rows(const cordahip_keyed_sig_batch* b, uint64_t a, uint64_t x, uint64_t y,
                               const SignLayout& l, const uint64_t* poff, uint32_t* hid, uint8_t* hsig, uint8_t* hsl,
                               uint8_t* hpre, uint8_t* hm, uint64_t* ho, uint32_t* hl) {
  const bool do_verify = !(b->flags & CORDAHIP_FLAG_IS_VALID);
  for (uint64_t i = x; i < y; i++) {
    const uint64_t o = b->msg_off[a + i], len = b->msg_off[a + i + 1] - o;
    const uint64_t so = b->sig_off[a + i], sl = b->sig_off[a + i + 1] - so;
    hid[i] = b->key_id[a + i];
    uint8_t st = CORDAHIP_STATUS_OK;
    if (sl <= 72) {
      if (sl) std::memcpy(hsig + i * 72, b->sig + so, sl);
      std::memset(hsig + i * 72 + sl, 0, 72 - sl);
      hsl[i] = (uint8_t)sl;
    } else {
      DerInt dr, ds;
      st = (len == 0 && do_verify) ? CORDAHIP_STATUS_EMPTY
           : der_decode_sig(b->sig + so, (uint32_t)std::min<uint64_t>(sl, 0xffffffffu), dr, ds)
               ? CORDAHIP_STATUS_BAD_SIG
               : CORDAHIP_STATUS_MALFORMED_SIG;
      std::memset(hsig + i * 72, 0, 72);
      hsl[i] = 72;
    }
    hpre[i] = st;
    pack_msg(b->msg, o, len, i, l, poff, hm, ho, hl);
  }
}

// ---- cordahip_rsa_verify_keyed launches (a batch that passed check_keyed_sig_batch) ----
// A launch is `rows` lanes of one width class W (64, 96 or 128 words), lanes[r] the
// batch's lane of row r. Its messages go out as a CSR of its rows: mo[rows + 1], the
// prefix of the lanes' message lengths from 0.
inline void rsa_keyed_msg_offsets(const cordahip_keyed_sig_batch* b, const uint64_t* lanes, uint64_t rows,
                                  uint64_t* mo) {
  mo[0] = 0;
  for (uint64_t r = 0; r < rows; r++) mo[r + 1] = mo[r] + (b->msg_off[lanes[r] + 1] - b->msg_off[lanes[r]]);
}
// Rows [x, y) of the launch: key ids, the signatures right-sized to zero-padded 4 W-byte
// slots with their lengths clamped to 4 W + 1, and each message at its CSR offset. A
// signature longer than the slot is longer than the modulus: its length alone decides
// it (BAD_SIG), none of its bytes is sent.
inline void rsa_keyed_pack_rows(const cordahip_keyed_sig_batch* b, const uint64_t* lanes, uint32_t W,
                                const uint64_t* mo, uint64_t x, uint64_t y, uint32_t* hid, uint8_t* hsig,
                                uint16_t* hsl, uint8_t* hm) {
  const uint64_t slot = 4ull * W;
  for (uint64_t r = x; r < y; r++) {
    const uint64_t i = lanes[r];
    hid[r] = b->key_id[i];
    const uint64_t sl = b->sig_off[i + 1] - b->sig_off[i], fit = sl <= slot ? sl : 0;
    uint8_t* row = hsig + r * slot;
    if (fit) std::memcpy(row, b->sig + b->sig_off[i], fit);
    std::memset(row + fit, 0, slot - fit);
    hsl[r] = (uint16_t)std::min<uint64_t>(sl, slot + 1);
    if (mo[r + 1] != mo[r]) std::memcpy(hm + mo[r], b->msg + b->msg_off[i], mo[r + 1] - mo[r]);
  }
}

}  // namespace rt
}  // namespace cordahip
