// Routing of ECDSA lanes to the keyed verifier (K15, ecdsa_route.hip): the match
// rule, the classes and the order of the routed partition, the tile geometry and
// the layout of the per-slot scratch, in one place. Usable from host and device
// (tests/test_ec_route_check.py builds tools/ec_route_check.cpp from it).
//
// The rule. While ECDSA routing is on and the device holds a live ECDSA key, lane i
// is keyed exactly when scheme[i] is 2 or 3 and equals the scheme of a live record
// of the device's ECDSA key table (ecdsa_vkey.hpp), and its key bytes are one of the
// two SEC1 encodings of that record's point: key_len[i] == 65 and the bytes are
// 04 || X || Y, or key_len[i] == 33 and the bytes are (02 | Y's low bit) || X, X and
// Y the point's canonical coordinates, 32 big-endian bytes each. Nothing but
// scheme, key_len and the key bytes enters the decision. A lane of the other scheme
// with the same bytes, 04 || X || p - Y, 04 || X || Y + p, a compressed encoding
// with the wrong parity, a hybrid encoding (06 / 07) and every other length miss and
// stay generic, which answers what it answers today. Of two live records of one
// scheme that hold the same point either may serve. Ed25519 records are in another
// table and are never seen.
//
// Where X and Y come from: entry (j = 0, d = 1) of a key's window table is the point
// itself, affine, canonical, in Montgomery form. The gather kernel, at the head of
// every routed enqueue, converts each live record's entry to plain big-endian bytes
// and writes (scheme, id, X[8], Y[8]) in slot order, and the count, into the scratch
// header; the key table keeps its size and its kernels.
//
// Classes of the routed partition: the generic engine's five (secp256k1 uncompressed
// / compressed, P-256 uncompressed / compressed, other), then keyed secp256k1, then
// keyed P-256. perm[n] holds the classes' runs in that order, so the generic list is
// perm[0 .. g), g = counts[0] + .. + counts[4], exactly what the unrouted partition
// would hold for those lanes (ecdsa_inv_kernel's counts[0..3] arithmetic is
// unchanged), the keyed secp256k1 run perm[g .. g + counts[5]) and the keyed P-256
// run behind it. counters: counts[7], then cursors[7] (the 64 bytes of EcWork::counters).
//
// The pass: a block owns a tile of kEcRouteTile lanes, visited in kEcRouteIter
// coalesced strides of 256. ecdsa_route_kernel loads the gathered records into LDS,
// writes route[i] (the key id, or kVkeyNoId) and totals the seven classes with one
// atomic per class per block; ecdsa_scatter_routed_kernel takes the class from
// route[i], reserves a wave's range of each class with one atomic and writes lane
// indices at range start + rank, iteration-major.
//
// Scratch of one ECDSA workspace slot (32-bit words; lane indices are 32-bit, so
// n <= kRouteMaxLanes):
//   [0] live records gathered  [1..15] unused
//   [16 ..)  kVkeySlots gathered records of kEcRouteRecWords words: scheme, id,
//            X (8 words: the 32 big-endian bytes in memory order), Y (8 words)
//   route[n] key id of lane i, or kVkeyNoId
// Bytes allocated for a batch of n lanes:
//   4 * (kEcRouteHdrWords + route_scratch_cap_lanes(n))
//     = 4,672 + 4 * (the power of two at or above n, at least 2^16)
// (route_scratch_cap_lanes: ed25519_route.hpp), so that batches of growing size do
// not reallocate it one by one.
#pragma once
#include <stdint.h>

#include "ecdsa_vkey.hpp"
#include "ed25519_route.hpp"

namespace cordahip {

static constexpr int kEcRouteRecWords = 18;  // a gathered record: scheme, id, X[8], Y[8] (72 bytes)
static constexpr int kEcRouteRecScheme = 0, kEcRouteRecId = 1, kEcRouteRecX = 2, kEcRouteRecY = 10;
static constexpr uint32_t kEcRouteCntLive = 0, kEcRouteRecBase = 16;
static constexpr uint32_t kEcRouteHdrWords = kEcRouteRecBase + kVkeySlots * kEcRouteRecWords;  // 1,168 words
static_assert(kEcRouteHdrWords * 4u == 4672u, "the header is 64 bytes and 64 records of 72");
VKEY_HD constexpr uint64_t ec_route_off_route() { return kEcRouteHdrWords; }
VKEY_HD constexpr uint64_t ec_route_scratch_words(uint64_t lanes) { return kEcRouteHdrWords + lanes; }

static constexpr int kEcRouteClasses = 7;  // the generic five, keyed secp256k1, keyed P-256
static constexpr int kEcRouteGenericClasses = 5;
static constexpr int kEcRouteIter = 16;  // = ecdsa.hip's kPartIter: the unrouted partition's tile
static constexpr int kEcRouteTile = 256 * kEcRouteIter;

// the generic engine's class of a lane (ecdsa.hip scheme_class)
VKEY_HD constexpr int ec_route_generic_class(uint8_t scheme, uint8_t key_len) {
  return scheme == 2 ? (key_len == 33 ? 1 : 0) : scheme == 3 ? (key_len == 33 ? 3 : 2) : 4;
}
// the routed class: a keyed lane (id != kVkeyNoId; its scheme is then 2 or 3) by curve
VKEY_HD constexpr int ec_route_class(uint8_t scheme, uint8_t key_len, uint32_t id) {
  return id == kVkeyNoId ? ec_route_generic_class(scheme, key_len) : (scheme == 2 ? 5 : 6);
}
// where the generic list ends and the keyed runs begin, from the seven counts
VKEY_HD uint64_t ec_route_generic_count(const uint32_t* counts) {
  uint64_t g = 0;
  for (int k = 0; k < kEcRouteGenericClasses; k++) g += counts[k];
  return g;
}
VKEY_HD uint64_t ec_route_keyed_start(const uint32_t* counts, uint32_t scheme) {
  return ec_route_generic_count(counts) + (scheme == 2 ? 0u : counts[5]);
}
VKEY_HD uint64_t ec_route_keyed_count(const uint32_t* counts, uint32_t scheme) { return counts[scheme == 2 ? 5 : 6]; }

// a record of the ECDSA key table (kEcVkeyRecWords words) that lanes may match
VKEY_HD bool ec_route_rec_live(const uint32_t* rec) {
  return rec[kEcVkeyRecLive] == 1u && rec[kEcVkeyRecId] != kVkeyNoId && vkey_gen(rec[kEcVkeyRecId]) != 0u &&
         (rec[kEcVkeyRecScheme] == 2u || rec[kEcVkeyRecScheme] == 3u);
}

// gathered record k: the point's plain coordinates as little-endian 32-bit words
// (x[7] the most significant) become 32 big-endian bytes each, kept in memory order
VKEY_HD void ec_route_put(uint32_t* gathered, uint32_t k, uint32_t scheme, uint32_t id, const uint32_t x[8],
                          const uint32_t y[8]) {
  uint32_t* o = gathered + k * kEcRouteRecWords;
  o[kEcRouteRecScheme] = scheme;
  o[kEcRouteRecId] = id;
  for (int q = 0; q < 8; q++) {
    o[kEcRouteRecX + q] = __builtin_bswap32(x[7 - q]);
    o[kEcRouteRecY + q] = __builtin_bswap32(y[7 - q]);
  }
}

// the live records of the table's kVkeySlots records gathered in slot order, each with
// its point's plain coordinates (points: per slot x[8], y[8], little-endian words);
// returns how many (the device does the same with one ballot, and takes the
// coordinates from the slot's window table: ecdsa_route.hip)
VKEY_HD uint32_t ec_route_gather(uint32_t* gathered, const uint32_t* recs, const uint32_t* points) {
  uint32_t k = 0;
  for (uint32_t s = 0; s < kVkeySlots; s++) {
    const uint32_t* rec = recs + s * kEcVkeyRecWords;
    if (!ec_route_rec_live(rec)) continue;
    ec_route_put(gathered, k++, rec[kEcVkeyRecScheme], rec[kEcVkeyRecId], points + s * 16, points + s * 16 + 8);
  }
  return k;
}

// The lane's key as the match reads it: byte 0, then bytes 1..32 (kx) and, for a
// 65-byte key, bytes 33..64 (ky) as words in memory order. key: the lane's 65-byte row.
VKEY_HD uint32_t ec_route_word(const uint8_t* p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

// the id of a gathered record whose scheme and point the lane's key bytes encode, or
// kVkeyNoId. Reads key[0 .. key_len) only, and only when key_len is 33 or 65.
VKEY_HD uint32_t ec_route_match(uint8_t scheme, uint8_t key_len, const uint8_t* key, const uint32_t* gathered,
                                uint32_t nlive) {
  if ((scheme != 2 && scheme != 3) || (key_len != 33 && key_len != 65) || nlive == 0) return kVkeyNoId;
  const uint32_t b0 = key[0];
  if (key_len == 65 ? b0 != 4u : (b0 & 0xfeu) != 2u) return kVkeyNoId;
  const uint32_t x0 = ec_route_word(key + 1);
  for (uint32_t k = 0; k < nlive; k++) {
    const uint32_t* r = gathered + k * kEcRouteRecWords;
    if (r[kEcRouteRecX] != x0 || r[kEcRouteRecScheme] != scheme) continue;
    uint32_t diff = 0;
    for (int q = 1; q < 8; q++) diff |= r[kEcRouteRecX + q] ^ ec_route_word(key + 1 + 4 * q);
    if (key_len == 65) {
      for (int q = 0; q < 8; q++) diff |= r[kEcRouteRecY + q] ^ ec_route_word(key + 33 + 4 * q);
    } else {
      // Y's low bit: the last of its 32 big-endian bytes, the top byte of word 7
      diff |= ((r[kEcRouteRecY + 7] >> 24) & 1u) ^ (b0 & 1u);
    }
    if (diff == 0) return r[kEcRouteRecId];
  }
  return kVkeyNoId;
}

// the lane that thread t (0..255) of the block owning `tile` visits in stride `it`
VKEY_HD constexpr uint64_t ec_route_tile_lane(uint64_t tile, int it, uint32_t t) {
  return tile * kEcRouteTile + (uint64_t)it * 256 + t;
}

}  // namespace cordahip
