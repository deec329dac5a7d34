// Required-signer coverage core, shared by the GPU kernel (tx.hip
// tx_cover_kernel, cordahip_tx_cover_device), the host pools of the covered
// signed-tx calls and the context-free host call (cover.cpp
// cordahip_cover_eval_host): the second half of SignedTransaction.verifySignatures,
//   getMissingSignatures     SignedTransaction.kt:102-108
//     tx.mustSign.filter { !it.isFulfilledBy(sigKeys) }   CryptoUtils.kt:79-82
//   CompositeKey.isFulfilledBy -> checkValidity, checkFulfilledBy   CompositeKey.kt:186-209, :110-122
//   checkConstraints / totalWeight                        CompositeKey.kt:73-85, :126-133
// over the wire form of include/cordahip.h (cordahip_cover): each required key
// is a post-order token stream over a shared key table.
//
// Written once for both sides: iterative (no recursion), no allocation, and no
// runtime-indexed private array -- the evaluation stack (one 8-byte slot per
// token: the subtree's weight in its parent, bit 32 = fulfilled) lives in
// caller-provided scratch, the tree's own slice stack[req_tok_off[r] ..), as
// K6 pmt_verify_kernel keeps its hashes. A required key that is a single leaf
// (every cash-issue transaction's) never touches the stack.
//
// Memory safety: token contents (key, nchild) are data and checked here; every
// offset is compared with the count its level declares before it is used
// (tx_req_off within nreq, req_tok_off within ntok, ckey_off within ckey_bytes:
// check_cover has rejected such a batch on the host paths; on the device path
// the offsets are the caller's contract, and a bad one costs the transaction a
// BAD_COVER instead of a read outside the arrays). Key bytes are read inside
// [ckey_off[k], ckey_off[k + 1]) and inside a signature's key range only; wide
// loads only from the dense 32-byte signature rows (16-byte aligned) and from
// a table key that is 32 bytes long at a 16-byte aligned address.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cordahip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define COVER_HD __host__ __device__ inline
#else
#define COVER_HD inline
#endif

namespace cordahip {
namespace cover {

constexpr uint32_t kMaxInt = 0x7fffffffu;  // a Java positive Int: 1 .. 2^31 - 1

// ---- how a transaction's signature keys are reached ---------------------------
// CSR keys (every host path; the device call with d_sig_key_off): signature s's
// key is key[key_off[s] .. key_off[s + 1]) under scheme[s] (scheme == nullptr:
// all Ed25519).
struct SigKeysCsr {
  const uint8_t* scheme;
  const uint8_t* key;
  const uint64_t* key_off;
  // some signature of [s0, s1) has scheme ks and the len bytes at k as its key
  COVER_HD bool any(uint64_t s0, uint64_t s1, uint8_t ks, const uint8_t* k, uint64_t len) const {
    for (uint64_t s = s0; s < s1; s++) {
      const uint8_t ss = scheme ? scheme[s] : (uint8_t)CORDAHIP_SCHEME_EDDSA_ED25519_SHA512;
      const uint64_t lo = key_off[s], hi = key_off[s + 1];
      if (ss != ks || hi < lo || hi - lo != len) continue;
      const uint8_t* p = key + lo;
      uint64_t i = 0;
      while (i < len && p[i] == k[i]) i++;
      if (i == len) return true;
    }
    return false;
  }
};

// Dense 32-byte rows (the *_ed25519_device calls' d_keys; 16-byte aligned):
// signature s's key is key[32 s .. 32 s + 32) under scheme[s] (nullptr: Ed25519).
struct SigKeysDense32 {
  const uint8_t* scheme;
  const uint8_t* key;
  COVER_HD bool any(uint64_t s0, uint64_t s1, uint8_t ks, const uint8_t* k, uint64_t len) const {
    if (len != 32) return false;
    // the table key, once: two 16-byte loads where its address allows, else bytes
    uint64_t w0, w1, w2, w3;
    if ((reinterpret_cast<uintptr_t>(k) & 15) == 0) {
      const void* k16 = __builtin_assume_aligned(k, 16);
      uint64_t w[4];
      __builtin_memcpy(w, k16, 32);
      w0 = w[0]; w1 = w[1]; w2 = w[2]; w3 = w[3];
    } else {
      w0 = w1 = w2 = w3 = 0;
      for (int i = 7; i >= 0; i--) {  // little-endian words, as the aligned loads read them
        w0 = (w0 << 8) | k[i];
        w1 = (w1 << 8) | k[8 + i];
        w2 = (w2 << 8) | k[16 + i];
        w3 = (w3 << 8) | k[24 + i];
      }
    }
    for (uint64_t s = s0; s < s1; s++) {
      const uint8_t ss = scheme ? scheme[s] : (uint8_t)CORDAHIP_SCHEME_EDDSA_ED25519_SHA512;
      if (ss != ks) continue;
      uint64_t r[4];
      __builtin_memcpy(r, __builtin_assume_aligned(key + 32 * s, 16), 32);
      if (((r[0] ^ w0) | (r[1] ^ w1) | (r[2] ^ w2) | (r[3] ^ w3)) == 0) return true;
    }
    return false;
  }
};

// Leaf fulfilment: some signature of the transaction has the same scheme byte,
// the same key length and the same key bytes (keysToCheck.contains(node),
// CompositeKey.kt:192; CryptoUtils.kt:79-82 for a plain key). kind: 0 not
// fulfilled, 1 fulfilled, 2 the key index or its table range is out of bounds.
template <class Sig>
COVER_HD int leaf_eval(const cordahip_cover& c, uint32_t key, const Sig& sig, uint64_t s0, uint64_t s1) {
  if (key >= c.nckey) return 2;
  const uint64_t lo = c.ckey_off[key], hi = c.ckey_off[(uint64_t)key + 1];
  if (hi < lo || hi > c.ckey_bytes) return 2;
  return sig.any(s0, s1, c.ckey_scheme[key], c.ckey + lo, hi - lo) ? 1 : 0;
}

constexpr uint64_t kFulfilledBit = 1ull << 32;

// ---- where a tree's evaluation stack lives ------------------------------------
// The tree's own slice of a scratch array of one slot per token (the GPU kernel,
// as K6 pmt_verify_kernel; a host caller that has one).
struct SliceStack {
  uint64_t* base;
  COVER_HD uint64_t* at(uint64_t k0, uint64_t) { return base + k0; }
};
// Host workers: a small inline buffer, the heap for a larger tree (kept for the
// worker's later trees). Plain keys never ask for it.
struct LocalStack {
  static constexpr uint64_t kInline = 64;
  uint64_t inl[kInline];
  uint64_t* heap = nullptr;
  uint64_t cap = 0;
  bool failed = false;
  LocalStack() = default;
  LocalStack(const LocalStack&) = delete;
  LocalStack& operator=(const LocalStack&) = delete;
#if !defined(__HIP_DEVICE_COMPILE__)
  ~LocalStack() { __builtin_free(heap); }
#endif
  COVER_HD uint64_t* at(uint64_t, uint64_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return nullptr;
#else
    if (n <= kInline) return inl;
    if (n > cap) {
      __builtin_free(heap);
      cap = 0;
      heap = n > SIZE_MAX / 8 ? nullptr : static_cast<uint64_t*>(__builtin_malloc((size_t)n * 8));
      if (heap) cap = n;
      else failed = true;  // the caller fails the call with OUT_OF_MEMORY: the verdict below is void
    }
    return heap;
#endif
  }
};

// One required key: CORDAHIP_REQ_FULFILLED / _MISSING / _MALFORMED. MALFORMED
// is what checkValidity would throw for (CompositeKey.kt:110-122 ->
// checkConstraints :73-85, totalWeight :126-133) plus a stream that is no tree;
// duplicate children (:74) are not looked for -- that needs structural subtree
// equality, and the JVM's constructor has enforced it.
template <class Sig, class Stack>
COVER_HD uint8_t req_eval(const cordahip_cover& c, uint64_t r, const Sig& sig, uint64_t s0, uint64_t s1,
                          Stack& stack) {
  const uint64_t k0 = c.req_tok_off[r], k1 = c.req_tok_off[r + 1];
  if (k1 <= k0 || k1 > c.ntok) return CORDAHIP_REQ_MALFORMED;  // empty (or not a range of tok)
  if (k1 - k0 == 1) {  // a plain key (a lone node has no children to stand on): no stack
    const cordahip_cover_tok tk = c.tok[k0];
    if (tk.nchild != 0) return CORDAHIP_REQ_MALFORMED;
    const int f = leaf_eval(c, tk.key, sig, s0, s1);
    return f == 2 ? CORDAHIP_REQ_MALFORMED : f ? CORDAHIP_REQ_FULFILLED : CORDAHIP_REQ_MISSING;
  }
  uint64_t* stk = stack.at(k0, k1 - k0);  // at most one slot per token: sp <= k - k0 before token k
  if (!stk) return CORDAHIP_REQ_MALFORMED;  // host only: the heap fallback failed (LocalStack::failed)
  uint64_t sp = 0;
  for (uint64_t k = k0; k < k1; k++) {
    const cordahip_cover_tok tk = c.tok[k];
    uint64_t slot = tk.weight;
    if (tk.nchild == 0) {
      const int f = leaf_eval(c, tk.key, sig, s0, s1);
      if (f == 2) return CORDAHIP_REQ_MALFORMED;
      if (f) slot |= kFulfilledBit;
    } else {
      const uint64_t n = tk.nchild;
      if (n < 2 || n > sp) return CORDAHIP_REQ_MALFORMED;                      // :77; not a tree
      if (tk.threshold == 0 || tk.threshold > kMaxInt) return CORDAHIP_REQ_MALFORMED;  // :79
      uint64_t total = 0, got = 0;
      for (uint64_t i = sp - n; i < sp; i++) {
        const uint64_t ch = stk[i];
        const uint64_t w = ch & 0xffffffffull;
        if (w == 0 || w > kMaxInt) return CORDAHIP_REQ_MALFORMED;  // :129 weight > 0
        total += w;
        if (total > kMaxInt) return CORDAHIP_REQ_MALFORMED;  // :130 Math.addExact
        if (ch & kFulfilledBit) got += w;
      }
      if (tk.threshold > total) return CORDAHIP_REQ_MALFORMED;  // :82
      sp -= n;
      if (got >= tk.threshold) slot |= kFulfilledBit;  // checkFulfilledBy :186-196
    }
    stk[sp++] = slot;
  }
  if (sp != 1) return CORDAHIP_REQ_MALFORMED;  // does not reduce to one value
  return (stk[0] & kFulfilledBit) ? CORDAHIP_REQ_FULFILLED : CORDAHIP_REQ_MISSING;  // the root's weight is ignored
}

// One transaction (include/cordahip.h "Per transaction, in this order"): a
// transaction that has already failed keeps its status and its entries are
// NOT_EVALUATED; otherwise every entry is evaluated on its own, the first
// MALFORMED one makes it BAD_COVER (filter runs to the end and the first invalid
// key throws before any missing set exists), else the first MISSING one that is
// not allowed to be missing makes it SIGNATURES_MISSING (SignedTransaction.kt:76-82).
template <class Sig, class Stack>
COVER_HD void tx_eval(const cordahip_cover& c, uint64_t t, uint8_t* tx_status, const uint64_t* tx_sig_off,
                      const Sig& sig, Stack& stack) {
  const uint64_t r0 = c.tx_req_off[t], r1 = c.tx_req_off[t + 1];
  const bool range_ok = r0 <= r1 && r1 <= c.nreq;
  c.first_missing[t] = -1;
  if (tx_status[t] != CORDAHIP_STATUS_OK) {
    if (range_ok)
      for (uint64_t r = r0; r < r1; r++) c.req_status[r] = CORDAHIP_REQ_NOT_EVALUATED;
    return;
  }
  if (!range_ok) {  // not a range of the required keys: nothing of it is read
    tx_status[t] = CORDAHIP_TX_BAD_COVER;
    return;
  }
  const uint64_t s0 = tx_sig_off[t], s1 = tx_sig_off[t + 1];
  int64_t first_mal = -1, first_miss = -1;
  for (uint64_t r = r0; r < r1; r++) {
    uint8_t st = req_eval(c, r, sig, s0, s1, stack);
    if (st == CORDAHIP_REQ_MISSING && c.req_flags && (c.req_flags[r] & 1)) st = CORDAHIP_REQ_MISSING_ALLOWED;
    c.req_status[r] = st;
    if (st == CORDAHIP_REQ_MALFORMED && first_mal < 0) first_mal = (int64_t)(r - r0);
    if (st == CORDAHIP_REQ_MISSING && first_miss < 0) first_miss = (int64_t)(r - r0);
  }
  if (first_mal >= 0) {
    tx_status[t] = CORDAHIP_TX_BAD_COVER;
    c.first_missing[t] = first_mal;
  } else if (first_miss >= 0) {
    tx_status[t] = CORDAHIP_TX_SIGNATURES_MISSING;
    c.first_missing[t] = first_miss;
  }
}

}  // namespace cover
}  // namespace cordahip
