// Routing of RSA rows to the keyed modular exponentiation (K20, rsa.hip): the match
// rule, the geometry of the route pass and the layout of the scratch it fills, in
// one place. Usable from host and device (tests/test_rsa_route_check.py builds
// tools/rsa_route_check.cpp from it).
//
// The rule. While RSA routing is on and the device's RSA key table (rsa_vkey.hpp)
// holds a live record, row i of a launch of width class W is keyed exactly when some
// live record has words == W, e == exp[i] and n[0 .. W) == mod[i][0 .. W), all W
// words. Nothing else enters the decision. A registered 2048-bit key whose modulus
// sits zero-padded in a 96- or 128-word row misses (its words is 64) and stays
// generic, which answers what it answers today. Of two live records with the same
// key either may serve. A cleared record is zero, id 0 is never issued, so it matches
// nothing. The row keeps its modulus, so the generic prep and check kernels serve
// routed rows unchanged: only the exponentiation between them differs.
//
// The pass (rsa_route_kernel): blocks of 256 threads, one lane per row, row = block *
// 256 + thread. Every block first gathers the live records' (id, words, e, n[0]) --
// 16 bytes each, at most 64 -- into LDS in slot order; a row compares the table's full
// n only against candidates that agree in words, e and n[0]. route[i] gets the key id
// or kVkeyNoId. The rows whose prep status is OK are compacted into two index lists,
// keyed and generic: a wave takes one ballot per list, reserves its range with one
// atomic per list and writes row indices at range start + rank, so a list holds each
// wave's rows in ascending order, the waves in the order their atomics landed. A row
// the prep decided needs no exponentiation and enters neither list. The cumulative
// totals count every row by match, decided by the prep or not.
//
// Scratch of one RSA workspace (32-bit words), sized by the workspace's row cap:
//   [0] keyed count  [1] generic count  [2..15] unused (the header: 64 bytes)
//   route[cap]    key id of row i of the launch, or kVkeyNoId
//   keyed[cap]    the keyed rows, keyed count of them
//   generic[cap]  the generic rows, generic count of them
// 64 + 12 * cap bytes. The two counts are cleared in front of every launch's route
// pass, on the launch's stream: launch k + 1 never reads launch k's counts.
#pragma once
#include <stdint.h>

#include "ed25519_route.hpp"
#include "rsa_vkey.hpp"

namespace cordahip {

static constexpr int kRsaRouteBlock = 256;     // rows per block of the route pass
static constexpr int kRsaRouteCandWords = 4;   // a gathered candidate: id, words, e, n[0]
static constexpr int kRsaRouteCandId = 0, kRsaRouteCandWordsW = 1, kRsaRouteCandE = 2, kRsaRouteCandN0 = 3;
static constexpr int kRsaRouteGroupsPerBlock = 32;  // rsa.hip: 8 lanes a row, 256 threads

static constexpr uint32_t kRsaRouteCntKeyed = 0, kRsaRouteCntGeneric = 1, kRsaRouteHdrWords = 16;
VKEY_HD constexpr uint64_t rsa_route_off_route(uint64_t) { return kRsaRouteHdrWords; }
VKEY_HD constexpr uint64_t rsa_route_off_keyed(uint64_t cap) { return kRsaRouteHdrWords + cap; }
VKEY_HD constexpr uint64_t rsa_route_off_generic(uint64_t cap) { return kRsaRouteHdrWords + 2 * cap; }
VKEY_HD constexpr uint64_t rsa_route_scratch_words(uint64_t cap) { return kRsaRouteHdrWords + 3 * cap; }

// a record of the RSA key table (rsa::kVkeyRecWords words) that rows may match
VKEY_HD bool rsa_route_rec_live(const uint32_t* rec) {
  const uint32_t id = rec[rsa::kVkeyRecIdWord], w = rec[rsa::kVkeyRecWordsWord];
  return id != 0u && id != kVkeyNoId && vkey_gen(id) != 0u && (w == 64u || w == 96u || w == 128u);
}

// the candidate entry of a live record
VKEY_HD void rsa_route_put(uint32_t* cand, uint32_t k, const uint32_t* rec) {
  uint32_t* o = cand + k * kRsaRouteCandWords;
  o[kRsaRouteCandId] = rec[rsa::kVkeyRecIdWord];
  o[kRsaRouteCandWordsW] = rec[rsa::kVkeyRecWordsWord];
  o[kRsaRouteCandE] = rec[rsa::kVkeyRecEWord];
  o[kRsaRouteCandN0] = rec[rsa::kVkeyRecNWord];
}

// the live records of the table's kVkeySlots records gathered in slot order; returns
// how many (the device does the same with one ballot: rsa.hip)
VKEY_HD uint32_t rsa_route_gather(uint32_t* cand, const uint32_t* tab) {
  uint32_t k = 0;
  for (uint32_t s = 0; s < kVkeySlots; s++) {
    const uint32_t* rec = tab + (size_t)s * rsa::kVkeyRecWords;
    if (rsa_route_rec_live(rec)) rsa_route_put(cand, k++, rec);
  }
  return k;
}

// the id of a live record whose class is W, whose exponent is e and whose modulus
// equals mod[0 .. W), or kVkeyNoId. Reads mod[0 .. W) only, the table only for
// candidates that agree in words, e and n[0] (a candidate's record is in its id's slot).
VKEY_HD uint32_t rsa_route_match(uint32_t W, uint32_t e, const uint32_t* mod, const uint32_t* cand, uint32_t ncand,
                                 const uint32_t* tab) {
  if (ncand == 0) return kVkeyNoId;
  const uint32_t n0 = mod[0];
  for (uint32_t k = 0; k < ncand; k++) {
    const uint32_t* c = cand + k * kRsaRouteCandWords;
    if (c[kRsaRouteCandN0] != n0 || c[kRsaRouteCandE] != e || c[kRsaRouteCandWordsW] != W) continue;
    const uint32_t* n = tab + (size_t)vkey_slot(c[kRsaRouteCandId]) * rsa::kVkeyRecWords + rsa::kVkeyRecNWord;
    uint32_t diff = 0;
    for (uint32_t q = 1; q < W; q++) diff |= n[q] ^ mod[q];
    if (diff == 0) return c[kRsaRouteCandId];
  }
  return kVkeyNoId;
}

// the row that thread t (0..255) of block `block` of the route pass visits
VKEY_HD constexpr uint64_t rsa_route_row(uint64_t block, uint32_t t) { return block * kRsaRouteBlock + t; }

// The indexed exponentiation kernels run grids sized for the launch's rows; group j of
// block `block` takes list position block * 32 + j. A block wholly past the list's
// count returns as a block; inside a live block the groups past the count run stand-ins.
VKEY_HD constexpr uint64_t rsa_route_idx_blocks(uint64_t rows) {
  return (rows + kRsaRouteGroupsPerBlock - 1) / kRsaRouteGroupsPerBlock;
}
VKEY_HD constexpr bool rsa_route_idx_block_live(uint64_t block, uint64_t count) {
  return block * kRsaRouteGroupsPerBlock < count;
}
VKEY_HD constexpr uint64_t rsa_route_idx_pos(uint64_t block, uint32_t group) {
  return block * kRsaRouteGroupsPerBlock + group;
}

// the rows of the launch that starts at row lo of a batch of n rows over a workspace of ws_rows rows
VKEY_HD constexpr uint64_t rsa_route_launch_rows(uint64_t ws_rows, uint64_t n, uint64_t lo) {
  return n - lo < ws_rows ? n - lo : ws_rows;
}

// K23 / K24: the batch's rows are known on the device only (count); the rows of the launch
// that holds rows lo .. lo + m of the host's bound, clipped to m (rsa.hip
// rsa_launch_count_kernel). The route pass clips what it reads once more (route_count_clip).
VKEY_HD constexpr uint64_t rsa_route_launch_count(uint64_t count, uint64_t lo, uint64_t m) {
  return count > lo ? (count - lo < m ? count - lo : m) : 0;
}

}  // namespace cordahip
