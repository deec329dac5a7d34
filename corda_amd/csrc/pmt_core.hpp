// Partial-Merkle-tree build core, shared by the GPU kernel (tx.hip
// pmt_build_kernel, K10) and the host fuzzer (tools/pmt_build_fuzz.cpp): what
// FilteredTransaction.buildMerkleTransaction does after the leaf hashes,
//   buildMerkleTransaction       MerkleTransaction.kt:121-128
//   MerkleTree.getMerkleTree     MerkleTree.kt:27-66 (padWithZeros to 2^k, zeroHash = 32 x 0x00)
//   PartialMerkleTree.build      PartialMerkleTree.kt:68-78
//   buildPartialTree             PartialMerkleTree.kt:100-125
// for one transaction: the included set (membership by HASH: root.hash in
// includeHashes), the count rule (includeHashes.size != usedHashes.size ->
// MerkleTreeException), the padded tree with every level kept, and the
// post-order token stream (0 IncludedLeaf, 1 Leaf, 2 Node) K6 reads.
//
// Written once for both sides: iterative (no recursion), no allocation, no
// runtime-indexed private array. A transaction's workspace is caller-provided:
//   up   the tree's levels above the leaves, level 1 first: at most 2 m hashes
//        (sum over j >= 1 of ceil(m / 2^j) <= m + ceil(log2 m) <= 2 m - 1 for m >= 2)
//   has  one byte per real node, the leaves first: at most 3 m bytes
//        (nonzero: an included leaf lies below the node)
// so transaction t's slices start at 2 * tx_leaf_off[t] and 3 * tx_leaf_off[t]:
// no scan. Positions right of a level's real nodes are the padding constants
// Z_j and are neither stored nor hashed. Hashes are 8 big-endian state words;
// the node hash and the Z_j table are template parameters (the device passes
// sha256_node and kZeroHash, the fuzzer cheap stand-ins).
//
// Memory safety: reads leaf[0 .. 8 m), include[0 .. m); writes up / has inside
// the bounds above, 32 bytes at txid, one entry each of ntok / status, and
// tokens only below min(cap, 2 pad(m) - 1) of the slot -- a slot smaller than
// the bound gets no token at all (kSlotTooSmall).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PMT_HD __host__ __device__ inline
#else
#define PMT_HD inline
#endif

namespace cordahip {
namespace pmt {

constexpr uint8_t kOk = 0;               // CORDAHIP_STATUS_OK
constexpr uint8_t kNoLeaves = 6;         // CORDAHIP_TX_NO_LEAVES
constexpr uint8_t kHashesNotInTree = 12; // CORDAHIP_TX_HASHES_NOT_IN_TREE
constexpr uint8_t kSlotTooSmall = 13;    // CORDAHIP_TX_TOK_SLOT_TOO_SMALL
constexpr uint8_t kTokIncluded = 0, kTokLeaf = 1, kTokNode = 2;

// Tokens the slot of an m-leaf transaction must hold: 2 pad(m) - 1, pad(m) the
// next power of two >= m (every padded position its own token: reached when all
// of a power-of-two m is flagged); 0 for m == 0. false: the bound does not fit.
PMT_HD bool slot_bound(uint64_t m, uint64_t* need) {
  *need = 0;
  if (m == 0) return true;
  if (m > (1ull << 62)) return false;
  uint64_t p = 1;
  while (p < m) p <<= 1;
  *need = 2 * p - 1;
  return true;
}

// real nodes of level j of an m-leaf tree (m >= 1, j < 64): ceil(m / 2^j)
PMT_HD uint64_t level_count(uint64_t m, int j) { return ((m - 1) >> j) + 1; }

// 8 state words at a 32-byte aligned address
PMT_HD void ld8(uint32_t w[8], const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* p4 = reinterpret_cast<const uint4*>(p);
  const uint4 a = p4[0], b = p4[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
#else
  for (int k = 0; k < 8; k++) w[k] = p[k];
#endif
}
PMT_HD void st8(uint32_t* p, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* p4 = reinterpret_cast<uint4*>(p);
  p4[0] = make_uint4(w[0], w[1], w[2], w[3]);
  p4[1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int k = 0; k < 8; k++) p[k] = w[k];
#endif
}
PMT_HD bool eq8(const uint32_t* a, const uint32_t* b) {
  uint32_t x[8], y[8], d = 0;
  ld8(x, a);
  ld8(y, b);
  for (int k = 0; k < 8; k++) d |= x[k] ^ y[k];
  return d == 0;
}
// state words -> the 32 bytes of a SecureHash (big-endian), any address:
// 16-byte stores where it allows (the device call's buffers are the caller's)
PMT_HD void st_be(uint8_t* dst, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    d4[0] = make_uint4(__builtin_bswap32(w[0]), __builtin_bswap32(w[1]), __builtin_bswap32(w[2]),
                       __builtin_bswap32(w[3]));
    d4[1] = make_uint4(__builtin_bswap32(w[4]), __builtin_bswap32(w[5]), __builtin_bswap32(w[6]),
                       __builtin_bswap32(w[7]));
    return;
  }
#endif
  for (int k = 0; k < 8; k++) {
    dst[4 * k] = (uint8_t)(w[k] >> 24);
    dst[4 * k + 1] = (uint8_t)(w[k] >> 16);
    dst[4 * k + 2] = (uint8_t)(w[k] >> 8);
    dst[4 * k + 3] = (uint8_t)w[k];
  }
}

// One transaction. leaf: its m leaf hashes; include: its m filter bytes; up / has:
// its workspace slices (above); cap: entries of its token slot, tok / tok_hash
// pointing at the slot's start (not dereferenced when no token is written).
// node(out, a, b): the node hash; zero(level, out): Z_level.
//
// Status decisions, in this order: m == 0 -> kNoLeaves (zero id, as K4 writes
// it); the id (= rootHash) is written for every m > 0; the count rule ->
// kHashesNotInTree (the reference's exception does not depend on any buffer, so
// it comes before the slot); cap < 2 pad(m) - 1 -> kSlotTooSmall; else kOk
// with the tokens. Every non-OK transaction has *ntok = 0.
template <class NodeHash, class ZeroHash>
PMT_HD void build_tx(uint64_t m, const uint32_t* leaf, const uint8_t* include, uint32_t* up, uint8_t* has,
                     uint64_t cap, uint8_t* tok, uint8_t* tok_hash, uint8_t* txid, uint64_t* ntok,
                     uint8_t* status, NodeHash node, ZeroHash zero) {
  *ntok = 0;
  uint32_t a[8], b[8], r[8];
  if (m == 0) {
    for (int k = 0; k < 8; k++) r[k] = 0;
    st_be(txid, r);
    *status = kNoLeaves;
    return;
  }
  // The included set: leaf i becomes an IncludedLeaf iff some flagged leaf has
  // its hash. A flagged leaf is its own witness; an unflagged one is compared
  // with the flagged ones.
  uint64_t nflag = 0, nincl = 0;
  for (uint64_t i = 0; i < m; i++) {
    const uint8_t f = include[i] != 0;
    has[i] = f;
    nflag += f;
  }
  nincl = nflag;
  if (nflag != 0 && nflag != m) {
    for (uint64_t i = 0; i < m; i++) {
      if (include[i] != 0) continue;
      for (uint64_t j = 0; j < m; j++) {
        if (include[j] == 0 || !eq8(leaf + 8 * i, leaf + 8 * j)) continue;
        has[i] = 1;
        nincl++;
        break;
      }
    }
  }
  // The padded tree, every level kept: each real node hashed once, its `has`
  // byte the OR of its children's.
  const uint32_t* cur = leaf;
  const uint8_t* hc = has;
  uint32_t* nxt = up;
  uint8_t* hn = has + m;
  uint64_t c = m, top_off = 0;  // top_off: the top level's first node in `up`
  int depth = 0;
  while (c > 1) {
    const uint64_t half = (c + 1) / 2;
    for (uint64_t i = 0; i < half; i++) {
      ld8(a, cur + 16 * i);
      uint8_t h = hc[2 * i];
      if (2 * i + 1 < c) {
        ld8(b, cur + 16 * i + 8);
        h |= hc[2 * i + 1];
      } else {
        zero(depth, b);  // the last real node pairs with the padding constant
      }
      node(r, a, b);
      st8(nxt + 8 * i, r);
      hn[i] = h;
    }
    if (depth > 0) top_off += c;
    cur = nxt;
    hc = hn;
    nxt += 8 * half;
    hn += half;
    c = half;
    depth++;
  }
  ld8(r, cur);
  st_be(txid, r);
  if (nincl != nflag) {
    *status = kHashesNotInTree;
    return;
  }
  uint64_t need;
  if (!slot_bound(m, &need) || cap < need) {
    *status = kSlotTooSmall;
    return;
  }
  // Post-order walk of the padded tree by (level, index); `uo` is the current
  // level's first node in `up` (levels >= 1). A node with no included leaf
  // below collapses to Leaf(its hash); a position right of its level's real
  // nodes is the padding-only subtree Leaf(Z_level).
  uint64_t n = 0, i = 0, uo = top_off;
  int j = depth;
  for (;;) {
    if (i >= level_count(m, j)) {
      zero(j, r);
      if (n < cap) {
        tok[n] = kTokLeaf;
        st_be(tok_hash + 32 * n, r);
      }
      n++;
    } else {
      const uint8_t h = j ? has[m + uo + i] : has[i];
      if (h && j) {  // descend to the left child
        j--;
        if (j) uo -= level_count(m, j);
        i *= 2;
        continue;
      }
      ld8(r, j ? up + 8 * (uo + i) : leaf + 8 * i);
      if (n < cap) {
        tok[n] = h ? kTokIncluded : kTokLeaf;
        st_be(tok_hash + 32 * n, r);
      }
      n++;
    }
    // (j, i) is complete: its right sibling next, or the parents it completes
    bool done = false;
    for (;;) {
      if (j == depth) {
        done = true;
        break;
      }
      if ((i & 1) == 0) {
        i++;
        break;
      }
      if (n < cap) tok[n] = kTokNode;
      n++;
      uo = j ? uo + level_count(m, j) : 0;
      j++;
      i >>= 1;
    }
    if (done) break;
  }
  *ntok = n;
  *status = kOk;
}

// Transaction t of a batch, as K10's lane runs it: its leaf range, its workspace
// slices and its token slot. The slot offsets of the device-resident call are
// only ever read here, so they are judged here: a slot that is reversed or
// reaches past ntok counts as empty (kSlotTooSmall for m > 0, and the slot's
// address is never formed into an access). The leaf-level offsets are the
// caller's contract (checked on the host forms by check_filtered_build_batch).
template <class NodeHash, class ZeroHash>
PMT_HD void build_lane(uint64_t t, const uint32_t* hashes, const uint64_t* tx_leaf_off, const uint8_t* include,
                       const uint64_t* tx_tok_off, uint64_t ntok, uint32_t* up, uint8_t* has, uint8_t* txid,
                       uint8_t* tok, uint8_t* tok_hash, uint64_t* tx_ntok, uint8_t* tx_status, NodeHash node,
                       ZeroHash zero) {
  const uint64_t lo = tx_leaf_off[t], hi = tx_leaf_off[t + 1];
  const uint64_t k0 = tx_tok_off[t], k1 = tx_tok_off[t + 1];
  const bool slot = k0 <= k1 && k1 <= ntok;
  const uint64_t cap = slot ? k1 - k0 : 0, at = slot ? k0 : 0;
  build_tx(hi - lo, hashes + lo * 8, include + lo, up + lo * 16, has + lo * 3, cap, tok + at, tok_hash + at * 32,
           txid + t * 32, tx_ntok + t, tx_status + t, node, zero);
}

}  // namespace pmt
}  // namespace cordahip
