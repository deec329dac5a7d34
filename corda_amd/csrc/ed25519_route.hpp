// Routing of Ed25519 lanes to the keyed verifier (K14, ed25519_route.hip): the
// match rule, the tile geometry of the partition pass and the layout of the
// per-slot scratch it fills, in one place. Usable from host and device
// (tests/test_ed_route_check.py builds tools/ed_route_check.cpp from it).
//
// A lane is keyed exactly when its 32 key bytes equal the Abyte of a live record of
// the device's verification-key table (ed25519_vkey.hpp: kVkeyRecAbyte, the canonical
// encoding the build kernel stored). Nothing else enters the decision: a
// non-canonical encoding of a registered point misses and stays generic, where K1
// decodes it to the same point. Two live records with equal bytes: either may serve.
//
// The pass: every block first gathers the live records (Abyte and id, 36 bytes each,
// at most 64) into LDS, in slot order. A block owns a tile of kRouteTile lanes,
// visited in kRouteIter coalesced strides of 256; a wave totals its kRouteIter
// ballots per list, reserves its range of each list with one atomic, and writes
// lane indices at range start + rank, iteration-major. The lists therefore hold each
// wave's lanes in ascending order, the waves in the order their atomics landed.
//
// Scratch of n lanes (32-bit words; lane indices are 32-bit, so n <= kRouteMaxLanes):
//   [0] keyed count  [1] generic count  [2..15] unused (the header: 64 bytes)
//   route[n]    key id of lane i, or kVkeyNoId
//   keyed[n]    the keyed lanes, keyed count of them
//   generic[n]  the others, generic count of them
// The layout follows the batch's n; the buffer behind it is allocated for
// route_scratch_cap_lanes(n) lanes (powers of two from kRouteMinLanes), so that batches
// of growing size do not reallocate it one by one.
#pragma once
#include <stdint.h>

#include "ed25519_vkey.hpp"

namespace cordahip {

static constexpr int kRouteRecWords = 9;  // a gathered record: Abyte (8 words), id
static constexpr int kRouteIter = 8;
static constexpr int kRouteTile = 256 * kRouteIter;
static constexpr uint64_t kRouteMaxLanes = 0xFFFFFFFFull;

static constexpr uint32_t kRouteCntKeyed = 0, kRouteCntGeneric = 1, kRouteHdrWords = 16;
VKEY_HD constexpr uint64_t route_off_route(uint64_t) { return kRouteHdrWords; }
VKEY_HD constexpr uint64_t route_off_keyed(uint64_t n) { return kRouteHdrWords + n; }
VKEY_HD constexpr uint64_t route_off_generic(uint64_t n) { return kRouteHdrWords + 2 * n; }
VKEY_HD constexpr uint64_t route_scratch_words(uint64_t n) { return kRouteHdrWords + 3 * n; }
static constexpr uint64_t kRouteMinLanes = 1ull << 16;  // 768 KiB of scratch
// lanes to allocate for: the power of two at or above n, at least kRouteMinLanes, at most kRouteMaxLanes
VKEY_HD constexpr uint64_t route_scratch_cap_lanes(uint64_t n) {
  uint64_t c = kRouteMinLanes;
  while (c < n) c <<= 1;
  return c < kRouteMaxLanes ? c : kRouteMaxLanes;
}

// a record of the key table (kVkeyRecWords words) that lanes may match
VKEY_HD bool route_rec_live(const uint32_t* rec) {
  return rec[kVkeyRecLive] == 1u && rec[kVkeyRecId] != kVkeyNoId && vkey_gen(rec[kVkeyRecId]) != 0u;
}

// the live records of the table's kVkeySlots records gathered in slot order; returns
// how many (the device does the same with one ballot: ed25519_route.hip)
VKEY_HD uint32_t route_gather(uint32_t* out, const uint32_t* recs) {
  uint32_t k = 0;
  for (uint32_t s = 0; s < kVkeySlots; s++) {
    const uint32_t* rec = recs + s * kVkeyRecWords;
    if (!route_rec_live(rec)) continue;
    for (int q = 0; q < 8; q++) out[k * kRouteRecWords + q] = rec[kVkeyRecAbyte + q];
    out[k * kRouteRecWords + 8] = rec[kVkeyRecId];
    k++;
  }
  return k;
}

// the id of a gathered record whose 32 bytes equal the key's, or kVkeyNoId
VKEY_HD uint32_t route_match(const uint32_t key[8], const uint32_t* gathered, uint32_t nlive) {
  for (uint32_t k = 0; k < nlive; k++) {
    const uint32_t* r = gathered + k * kRouteRecWords;
    if (r[0] != key[0]) continue;
    uint32_t diff = 0;
    for (int q = 1; q < 8; q++) diff |= r[q] ^ key[q];
    if (diff == 0) return r[8];
  }
  return kVkeyNoId;
}

// K24, the counted instances of the three families' route passes: a row count read
// from device memory is the caller's data, so it is clipped to the bound the launch
// and its scratch were sized for before anything is indexed
VKEY_HD constexpr uint64_t route_count_clip(uint64_t count, uint64_t bound) { return count < bound ? count : bound; }

// the lane that thread t (0..255) of the block owning `tile` visits in stride `it`
VKEY_HD constexpr uint64_t route_tile_lane(uint64_t tile, int it, uint32_t t) {
  return tile * kRouteTile + (uint64_t)it * 256 + t;
}
// a lane's rank among the set lanes of its wave's ballot
VKEY_HD uint32_t route_rank(uint64_t ballot, uint32_t lane) {
  const uint64_t below = ballot & ((1ull << lane) - 1);
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popcll(below);
#else
  return (uint32_t)__builtin_popcountll(below);
#endif
}

// The generic engine runs over the generic list in workspace chunks of m lanes from
// list position base; the chunk's lanes once the count is known (0: wholly past it).
VKEY_HD uint64_t route_chunk_lanes(uint64_t count, uint64_t base, uint64_t m) {
  return base >= count ? 0 : (count - base < m ? count - base : m);
}

}  // namespace cordahip
