// Mixed-scheme signature batches packed on the GPU (K23, sig_pack.hip): the per-lane
// rule, the classes, the tile geometry of the three passes, the counter block and the
// row writers, in one place. Usable from host and device: pack_rows.hpp (the host
// packer) takes its decisions from the rule below, sig_pack.hip runs it one lane per
// thread, and tools/sig_pack_check.cpp replays the passes with these functions on the
// CPU (tests/test_sig_pack_check.py). Everything takes raw pointers and lengths.
//
// The rule of lane i (CSR key and signature ranges, a scheme byte, a message length):
//   ranges_ok          the ranges are non-decreasing and inside the declared buffers;
//                      else the lane is kBad and not one byte of it is read
//   lane_rule          Crypto.kt's checks that need no arithmetic, in the host's order:
//                      ECDSA key length (BAD_KEY), RSA key decode (BAD_KEY / UNSUPPORTED,
//                      then EMPTY, then BAD_SIG for a signature longer than the modulus;
//                      UNSUPPORTED outright without the RSA flag), other schemes
//                      (UNSUPPORTED), Ed25519 key length (BAD_KEY): kDirect with the
//                      status, or the class whose verifier decides the lane
//   ed_pre / ec_pre    the pre-status a row of those classes carries
//
// The passes, each over tiles of kTile lanes (a block of 256 threads visits its tile in
// kIter strides of 256, so a wave's 64 lanes are consecutive lanes of the batch):
//   count    classify every lane, keep its code byte (count index | status << 4), and write
//            the block's kCounts totals
//   scan     per count, the exclusive prefix of the block totals and the batch total
//   pack     a lane's row within its class = the block's prefix + the lane's rank among
//            the block's lanes of the class (wave ballots, per-segment totals in LDS):
//            a stable partition, rows keep lane order. Rows, pre-statuses, lane_of_row
//            and msg_row lists are written; kDirect / kBad lanes get their status at once.
// No pass waits for another workgroup and nothing is read back: the host sizes every
// launch for the upper bound n, the verifiers read the class counts from the counter
// block (the K14 / K15 / K20 convention: list lengths are known on the device only).
//
// ECDSA rows are one run in lane order; the generic engine wants them partitioned by
// curve and key form, so the four ECDSA sub-counts are kept apart and the pack pass
// also writes perm[] (ecdsa_route.hpp: the runs of the engine's classes 0..3 over the
// rows), and the counter block carries the engine's 14-word counters.
#pragma once
#include <stdint.h>

#include "der.hpp"
#include "rsa_key.hpp"

namespace cordahip {
namespace sigpack {

// ---- classes, statuses, counters ---------------------------------------------------
enum : uint32_t { kDirect = 0, kEd = 1, kEc = 2, kRsa0 = 3, kRsa1 = 4, kRsa2 = 5, kBad = 6, kClasses = 7 };
// the counts the passes keep: the ECDSA class as the generic engine's four sub-classes
// (secp256k1 uncompressed / compressed, P-256 uncompressed / compressed)
enum : uint32_t { kCntDirect = 0, kCntEd = 1, kCntEc0 = 2, kCntRsa0 = 6, kCntBad = 9, kCounts = 10 };

static constexpr uint8_t kStOk = 0, kStBadSig = 1, kStMalformedSig = 2, kStBadKey = 3, kStUnsupported = 4,
                         kStEmpty = 5, kStBadRange = 19;  // CORDAHIP_STATUS_*
static constexpr uint8_t kSchemeRsa = 1, kSchemeK1 = 2, kSchemeR1 = 3, kSchemeEd = 4;  // CORDAHIP_SCHEME_*

static constexpr int kIter = 4;
static constexpr int kTile = 256 * kIter;
static constexpr int kSegs = 4 * kIter;  // (stride, wave) pairs of a tile, in lane order
static constexpr uint64_t kMaxLanes = 1ull << 31;  // n at or above it: 32-bit indices no longer do

CHD constexpr uint64_t tiles(uint64_t n) { return (n + kTile - 1) / kTile; }
// the lane that thread t (0..255) of the block owning `tile` visits in stride `it`
CHD constexpr uint64_t tile_lane(uint64_t tile, int it, uint32_t t) { return tile * kTile + (uint64_t)it * 256 + t; }
CHD constexpr int seg_of(int it, uint32_t t) { return it * 4 + (int)(t >> 6); }

// The counter block (32-bit words), followed at once by iota[n] (iota[i] = i):
//   [kHdrClass + c]  lanes of class c (7 words)
//   [kHdrRaw + k]    the kCounts totals as the scan left them
//   [kHdrEc ..)      the ECDSA engine's counters: counts[7] (0..3 the sub-classes, the rest
//                    zero), cursors[7]
//   [kHdrEd ..)      a header of ed25519_route.hpp's scratch (16 words, word 1 = the
//                    Ed25519 rows); the list behind it is iota: the engine's indexed
//                    instance then runs over rows 0 .. count
static constexpr uint32_t kHdrClass = 0, kHdrRaw = 8, kHdrEc = 20, kHdrEd = 48, kHdrWords = 64;
static constexpr uint32_t kHdrEdCount = kHdrEd + 1;

CHD constexpr uint32_t rsa_words(uint32_t cls) { return 64u + 32u * (cls - kRsa0); }
// An RSA key of class c holds its modulus: more than 128 / 256 / 384 bytes of DER. The
// host knows key_bytes, so a class whose lanes' key ranges are disjoint has at most
// key_bytes / that many rows, and its buffers are sized for that. The offsets are the
// caller's device data, though: ranges may overlap (many lanes over one key's bytes), and
// then a class can have more lanes than rows. Such a lane, at or past the bound in lane
// order, is a bad-range lane (kStBadRange, nothing of it packed), and the class count the
// verifiers, the gather and the scatter read is clipped to the bound (derive_header).
CHD constexpr uint64_t rsa_min_key_bytes(uint32_t cls) { return cls == kRsa0 ? 131u : cls == kRsa1 ? 260u : 388u; }
CHD constexpr uint64_t rsa_cap_rows(uint32_t cls, uint64_t n, uint64_t key_bytes) {
  return key_bytes / rsa_min_key_bytes(cls) < n ? key_bytes / rsa_min_key_bytes(cls) : n;
}

// which of the kCounts a lane of class cls adds to (ECDSA: by scheme and key length)
CHD constexpr uint32_t count_of(uint32_t cls, uint8_t scheme, uint64_t key_len) {
  return cls == kDirect ? kCntDirect
         : cls == kEd   ? kCntEd
         : cls == kEc   ? kCntEc0 + (scheme == kSchemeK1 ? 0u : 2u) + (key_len == 33 ? 1u : 0u)
         : cls == kBad  ? kCntBad
                        : kCntRsa0 + (cls - kRsa0);
}
CHD constexpr uint32_t class_of_count(uint32_t ci) {
  return ci == kCntDirect ? kDirect : ci == kCntEd ? kEd : ci < kCntRsa0 ? kEc : ci == kCntBad ? kBad : kRsa0 + (ci - kCntRsa0);
}
// a lane's code byte between the count and the pack pass: its count index and, for a
// kDirect lane, its status (0..5; a kBad lane's is kStBadRange)
CHD constexpr uint8_t code_of(uint32_t ci, uint8_t status) { return (uint8_t)(ci | (uint32_t)status << 4); }
CHD constexpr uint32_t code_count(uint8_t code) { return code & 15u; }
CHD constexpr uint8_t code_status(uint8_t code) { return code_count(code) == kCntBad ? kStBadRange : (uint8_t)(code >> 4); }

// ---- the rule ------------------------------------------------------------------------
// the lane's ranges, before any byte of it is read
CHD constexpr bool ranges_ok(uint64_t k0, uint64_t k1, uint64_t key_bytes, uint64_t s0, uint64_t s1,
                             uint64_t sig_bytes) {
  return !(k1 < k0 || k1 > key_bytes || s1 < s0 || s1 > sig_bytes);
}

// Ed25519 row: the Crypto.doVerify require()s, then the engine's length check
CHD constexpr uint8_t ed_pre(bool do_verify, uint64_t sig_len, uint64_t msg_len) {
  return do_verify && (sig_len == 0 || msg_len == 0) ? kStEmpty : sig_len != 64 ? kStMalformedSig : kStOk;
}

// ECDSA row: a signature longer than the 72-byte slot holds no r, s < n, so the DER
// rules alone decide it (BC: well-formed -> false, else SignatureException); the kernel
// still decodes the key first, so key errors keep precedence. Reads sig[0 .. sig_len).
CHD uint8_t ec_pre(bool do_verify, const uint8_t* sig, uint64_t sig_len, uint64_t msg_len) {
  if (sig_len <= 72) return kStOk;
  if (msg_len == 0 && do_verify) return kStEmpty;
  DerInt dr, ds;
  return der_decode_sig(sig, (uint32_t)(sig_len < 0xffffffffu ? sig_len : 0xffffffffu), dr, ds) ? kStBadSig
                                                                                             : kStMalformedSig;
}

// What is decided of an RSA lane without arithmetic: BAD_KEY / UNSUPPORTED from the key
// (strict RSAPublicKey decode), then EMPTY under doVerify rules, then BAD_SIG for a
// signature longer than the modulus (PSSSigner: false); kRsaToDevice with kv filled for
// the lanes whose verdict needs the arithmetic. Reads key[0 .. key_len).
static constexpr uint8_t kRsaToDevice = 0xff;
CHD uint8_t rsa_pre(const uint8_t* key, uint64_t key_len, uint64_t sig_len, uint64_t msg_len, bool do_verify,
                    rsa::KeyView& kv) {
  const uint8_t ks = rsa::parse_public_key_view(key, key_len, kv);
  if (ks != rsa::kOk) return ks;
  if (do_verify && (sig_len == 0 || msg_len == 0)) return kStEmpty;  // Crypto.kt:475-476
  if (sig_len > (kv.bits + 7) / 8) return kStBadSig;
  return kRsaToDevice;
}

struct Lane {
  uint32_t cls;    // kDirect, kEd, kEc, kRsa0 + width class
  uint8_t status;  // kDirect: the lane's status
};
// lane whose ranges are in order; kv is filled for the RSA classes
CHD Lane lane_rule(uint8_t scheme, const uint8_t* key, uint64_t key_len, uint64_t sig_len, uint64_t msg_len,
                   bool do_verify, bool rsa_on, rsa::KeyView& kv) {
  if (scheme == kSchemeK1 || scheme == kSchemeR1) {
    if (key_len != 33 && key_len != 65) return Lane{kDirect, kStBadKey};  // ECCurve.decodePoint: invalid point encoding
    return Lane{kEc, kStOk};
  }
  if (scheme == kSchemeRsa && rsa_on) {
    const uint8_t st = rsa_pre(key, key_len, sig_len, msg_len, do_verify, kv);
    if (st == kRsaToDevice) return Lane{kRsa0 + (kv.words / 32 - 2), kStOk};
    return Lane{kDirect, st};
  }
  if (scheme != kSchemeEd) return Lane{kDirect, kStUnsupported};  // Crypto.kt:474 require(isSupportedSignatureScheme)
  if (key_len != 32) return Lane{kDirect, kStBadKey};             // EdDSAPublicKeySpec: "public-key length is wrong"
  return Lane{kEd, kStOk};
}

// ---- the row writers -------------------------------------------------------------------
// Sources sit at arbitrary addresses (CSR offsets): they are read byte by byte, never
// past their length. Rows whose size is a multiple of 4 are written as words.
CHD uint32_t le32_clipped(const uint8_t* p, uint32_t at, uint32_t len) {  // bytes at .. at + 3 of p[0 .. len), zero past it
  uint32_t w = 0;
  for (uint32_t q = 0; q < 4; q++)
    if (at + q < len) w |= (uint32_t)p[at + q] << (8 * q);
  return w;
}

// Ed25519: the 32 key bytes and -- pre OK (sig_len 64) -- the 64 signature bytes; else a zero row
CHD void put_ed_row(const uint8_t* key, const uint8_t* sig, uint8_t pre, uint32_t* krow, uint32_t* srow) {
  for (uint32_t k = 0; k < 8; k++) krow[k] = le32_clipped(key, 4 * k, 32);
  for (uint32_t k = 0; k < 16; k++) srow[k] = pre == kStOk ? le32_clipped(sig, 4 * k, 64) : 0u;
}

// ECDSA: the key in its 65-byte slot, the DER signature in its 72-byte slot, zero-padded;
// a signature longer than the slot (pre from ec_pre) gets a zero slot of length 72
CHD void put_ec_row(const uint8_t* key, uint32_t key_len, const uint8_t* sig, uint64_t sig_len, uint8_t* krow,
                    uint8_t* key_len_out, uint8_t* srow, uint8_t* sig_len_out) {
  for (uint32_t k = 0; k < 65; k++) krow[k] = k < key_len ? key[k] : (uint8_t)0;
  *key_len_out = (uint8_t)key_len;
  const uint32_t sl = sig_len <= 72 ? (uint32_t)sig_len : 0u;
  for (uint32_t k = 0; k < 72; k++) srow[k] = k < sl ? sig[k] : (uint8_t)0;
  *sig_len_out = sig_len <= 72 ? (uint8_t)sig_len : (uint8_t)72;
}

// RSA, class of W words: the modulus as W little-endian words, e, the signature as it
// came (big-endian, sig_len <= ceil(bits / 8) <= 4 W) at the head of its 4 W-byte slot
CHD void put_rsa_row(const rsa::KeyView& kv, const uint8_t* sig, uint32_t sig_len, uint32_t W, uint32_t* mod,
                     uint32_t* exp, uint32_t* srow, uint16_t* sig_len_out) {
  for (uint32_t k = 0; k < W; k++) mod[k] = rsa::key_view_word(kv, k);
  *exp = kv.e;
  for (uint32_t k = 0; k < W; k++) srow[k] = le32_clipped(sig, 4 * k, sig_len);
  *sig_len_out = (uint16_t)sig_len;
}

// ---- a batch and its packed rows ----------------------------------------------------------
// The input (device memory on the GPU): CSR keys and signatures, a scheme byte per lane,
// dense message rows of msg_len bytes and -- msg_row non-null -- the row each lane signs
// (null: lane i signs row i).
struct In {
  const uint8_t* scheme;
  const uint8_t* key;
  const uint64_t* key_off;
  uint64_t key_bytes;
  const uint8_t* sig;
  const uint64_t* sig_off;
  uint64_t sig_bytes;
  const uint32_t* msg_row;
  uint64_t msg_rows;
  uint32_t msg_len;
  uint64_t n;
  uint32_t do_verify, rsa_on;
};
// The output: every array holds its class's upper bound of rows (n; an RSA class
// rsa_cap_rows(...), null without the RSA flag). lane[r]: the batch's lane of row r;
// msg[r]: its message row.
struct Out {
  uint32_t* hdr;     // kHdrWords + n: the counter block and iota
  uint8_t* code;     // n
  uint32_t* btot;    // kCounts * tiles(n): block totals, count-major
  uint32_t* boff;    // the same, scanned
  uint8_t* status;   // n: the caller's; kDirect / kBad lanes are written by the pack pass
  uint32_t *ed_key, *ed_sig;  // 8 / 16 words a row
  uint8_t* ed_pre;
  uint32_t *ed_lane, *ed_msg;
  uint8_t *ec_scheme, *ec_key, *ec_key_len, *ec_sig, *ec_sig_len, *ec_pre;  // 65- / 72-byte slots
  uint32_t *ec_lane, *ec_msg, *ec_perm;
  uint32_t *rsa_mod[3], *rsa_exp[3], *rsa_sig[3];  // W / 1 / W words a row
  uint16_t* rsa_sig_len[3];
  uint8_t* rsa_pre[3];
  uint32_t *rsa_lane[3], *rsa_msg[3];
  uint64_t rsa_cap[3];
};

// the count pass of lane i < n: its code byte
CHD uint8_t count_lane(const In& in, uint64_t i) {
  const uint64_t k0 = in.key_off[i], k1 = in.key_off[i + 1], s0 = in.sig_off[i], s1 = in.sig_off[i + 1];
  const uint64_t mr = in.msg_row ? in.msg_row[i] : i;
  if (!ranges_ok(k0, k1, in.key_bytes, s0, s1, in.sig_bytes) || mr >= in.msg_rows) return code_of(kCntBad, 0);
  rsa::KeyView kv;
  const uint8_t sch = in.scheme[i];
  const Lane l = lane_rule(sch, in.key + k0, k1 - k0, s1 - s0, in.msg_len, in.do_verify != 0, in.rsa_on != 0, kv);
  return code_of(count_of(l.cls, sch, k1 - k0), l.status);
}

// the pack pass of lane i < n with code byte `code`: row `row` of its class (ECDSA:
// position perm_pos of perm too). An RSA lane at or past its class's bound (overlapping
// key ranges: rsa_cap_rows) writes no row and gets kStBadRange; returns false for it.
CHD bool pack_lane(const In& in, const Out& out, uint64_t i, uint8_t code, uint64_t row, uint64_t perm_pos) {
  out.hdr[kHdrWords + i] = (uint32_t)i;
  const uint32_t cls = class_of_count(code_count(code));
  if (cls == kDirect || cls == kBad) {
    out.status[i] = code_status(code);
    return true;
  }
  const uint64_t k0 = in.key_off[i], kl = in.key_off[i + 1] - k0, s0 = in.sig_off[i], sl = in.sig_off[i + 1] - s0;
  const uint32_t mr = in.msg_row ? in.msg_row[i] : (uint32_t)i;
  const bool dv = in.do_verify != 0;
  if (cls == kEd) {
    const uint8_t pre = ed_pre(dv, sl, in.msg_len);
    put_ed_row(in.key + k0, in.sig + s0, pre, out.ed_key + row * 8, out.ed_sig + row * 16);
    out.ed_pre[row] = pre;
    out.ed_lane[row] = (uint32_t)i;
    out.ed_msg[row] = mr;
    return true;
  }
  if (cls == kEc) {
    out.ec_scheme[row] = in.scheme[i];
    put_ec_row(in.key + k0, (uint32_t)kl, in.sig + s0, sl, out.ec_key + row * 65, out.ec_key_len + row,
               out.ec_sig + row * 72, out.ec_sig_len + row);
    out.ec_pre[row] = ec_pre(dv, in.sig + s0, sl, in.msg_len);
    out.ec_lane[row] = (uint32_t)i;
    out.ec_msg[row] = mr;
    out.ec_perm[perm_pos] = (uint32_t)row;
    return true;
  }
  const uint32_t c = cls - kRsa0, W = rsa_words(cls);
  if (row >= out.rsa_cap[c]) {
    out.status[i] = kStBadRange;
    return false;
  }
  rsa::KeyView kv;
  (void)rsa::parse_public_key_view(in.key + k0, kl, kv);  // kOk: the count pass classified the lane
  put_rsa_row(kv, in.sig + s0, (uint32_t)sl, W, out.rsa_mod[c] + row * W, out.rsa_exp[c] + row, out.rsa_sig[c] + row * W,
              out.rsa_sig_len[c] + row);
  out.rsa_pre[c][row] = kStOk;
  out.rsa_lane[c][row] = (uint32_t)i;
  out.rsa_msg[c][row] = mr;
  return true;
}

// the counter block's derived words from the scan's totals (the pack pass, one thread);
// an RSA class's count is clipped to its rows (rsa_cap), the lanes past them are counted bad
CHD void derive_header(uint32_t* hdr, const uint64_t* rsa_cap) {
  const uint32_t* raw = hdr + kHdrRaw;
  hdr[kHdrClass + kDirect] = raw[kCntDirect];
  hdr[kHdrClass + kEd] = raw[kCntEd];
  hdr[kHdrClass + kEc] = raw[kCntEc0] + raw[kCntEc0 + 1] + raw[kCntEc0 + 2] + raw[kCntEc0 + 3];
  uint32_t over = 0;
  for (uint32_t c = 0; c < 3; c++) {
    const uint32_t have = raw[kCntRsa0 + c], fit = have < rsa_cap[c] ? have : (uint32_t)rsa_cap[c];
    hdr[kHdrClass + kRsa0 + c] = fit;
    over += have - fit;
  }
  hdr[kHdrClass + kBad] = raw[kCntBad] + over;
  for (uint32_t k = 0; k < 14; k++) hdr[kHdrEc + k] = k < 4 ? raw[kCntEc0 + k] : 0u;
  for (uint32_t k = 0; k < 16; k++) hdr[kHdrEd + k] = k == 1 ? raw[kCntEd] : 0u;
}

}  // namespace sigpack
}  // namespace cordahip
