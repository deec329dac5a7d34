// CSR validation at the C-ABI (ABI 4). Every offset array the host code indexes
// is checked before the host reads through it: offsets non-decreasing, the last
// one within the buffer length the caller declares, consecutive levels
// consistent (a transaction's leaves / items / signatures are ranges of the next
// level's arrays). A violation is CORDAHIP_ERR_INVALID_ARG, never a read outside
// the caller's buffers -- the reference turns bad input into an exception, not a
// crash (Crypto.kt:472-483, SignedTransaction.kt:37-39).
// The transaction-level batches are checked whole before any enqueue
// (check_txid_batch ...: a parallel pass over their offset arrays); the generic
// signature batch's per-lane offsets are checked in the classification pass
// that reads them anyway (pack_rows.hpp classify: a chunk with a bad lane is
// neither packed nor enqueued, the batch fails). No HIP here: tools/csr_fuzz.cpp
// runs this code and the per-lane classify/pack under ASan/UBSan on the CPU.
#pragma once
#include <stdint.h>

#include <atomic>

#include "../../include/cordahip.h"
#include "pmt_core.hpp"

namespace cordahip {
namespace rt {

// off[a..b] non-decreasing and off[b] <= limit. par(n, grain, fn(lo, hi)) runs
// fn over [0, n) in pieces (the context's host pool, or a serial loop).
template <class Par>
bool csr_ok(Par&& par, const uint64_t* off, uint64_t a, uint64_t b, uint64_t limit) {
  if (b < a || !off) return false;
  if (off[b] > limit) return false;
  std::atomic<bool> ok{true};
  par(b - a, 1u << 16, [&](uint64_t x, uint64_t y) {
    for (uint64_t i = a + x; i < a + y; i++)
      if (off[i] > off[i + 1]) {
        ok.store(false, std::memory_order_relaxed);
        return;
      }
  });
  return ok.load();
}

// the leaf level of a txid batch: tx_leaf_off[0..ntx] non-decreasing and within
// nleaves, and the leaves it spans inside leaf_bytes (leaf_off over them
// non-decreasing, the last <= leaf_bytes_len)
template <class Par>
bool check_txid_batch(Par&& par, const cordahip_txid_batch* b) {
  if (b->ntx == 0) return true;
  if (!b->tx_leaf_off || !b->leaf_off) return false;
  if (!csr_ok(par, b->tx_leaf_off, 0, b->ntx, b->nleaves)) return false;
  return csr_ok(par, b->leaf_off, b->tx_leaf_off[0], b->tx_leaf_off[b->ntx], b->leaf_bytes_len);
}

// the signature level of a signed-tx batch: tx_sig_off[0..ntx] non-decreasing and
// within nsig; key_off / sig_off over the signatures it spans inside key_bytes /
// sig_bytes (the per-lane classification checks them again as it reads them)
template <class Par>
bool check_sig_level(Par&& par, uint64_t ntx, const uint64_t* tx_sig_off, uint64_t nsig, const uint64_t* key_off,
                     uint64_t key_bytes, const uint64_t* sig_off, uint64_t sig_bytes) {
  if (ntx == 0) return true;
  if (!tx_sig_off || !csr_ok(par, tx_sig_off, 0, ntx, nsig)) return false;
  const uint64_t s0 = tx_sig_off[0], s1 = tx_sig_off[ntx];
  if (s0 == s1) return true;
  return csr_ok(par, key_off, s0, s1, key_bytes) && csr_ok(par, sig_off, s0, s1, sig_bytes);
}

// the item level of a component batch: tx_item_off[0..ntx] non-decreasing and
// within n_items (payload offsets are bounds-checked per item by the encoder)
template <class Par>
bool check_txcomp_batch(Par&& par, const cordahip_txcomp_batch* c) {
  if (c->ntx == 0) return true;
  return c->tx_item_off && csr_ok(par, c->tx_item_off, 0, c->ntx, c->n_items);
}

// a filtered-tx batch: the leaf level as in check_txid_batch, the token level
// tx_tok_off[0..ntx] non-decreasing and within ntok
template <class Par>
bool check_filtered_batch(Par&& par, const cordahip_filtered_tx_batch* b) {
  if (b->ntx == 0) return true;
  if (!b->tx_leaf_off || !b->leaf_off || !b->tx_tok_off) return false;
  if (!csr_ok(par, b->tx_leaf_off, 0, b->ntx, b->nleaves)) return false;
  if (!csr_ok(par, b->leaf_off, b->tx_leaf_off[0], b->tx_leaf_off[b->ntx], b->leaf_bytes_len)) return false;
  return csr_ok(par, b->tx_tok_off, 0, b->ntx, b->ntok);
}

// a filtered-tx build batch: the leaf level as in check_txid_batch; the token
// slots tx_tok_off[0..ntx] non-decreasing and within ntok; every transaction's
// slot at least 2 pad(m_t) - 1 tokens (pmt_core.hpp slot_bound: 0 for no
// leaves; an m_t whose bound does not fit in 64 bits is rejected)
template <class Par>
bool check_filtered_build_batch(Par&& par, const cordahip_filtered_build_batch* b) {
  if (b->ntx == 0) return true;
  if (!b->tx_leaf_off || !b->leaf_off || !b->tx_tok_off) return false;
  if (!csr_ok(par, b->tx_leaf_off, 0, b->ntx, b->nleaves)) return false;
  if (!csr_ok(par, b->leaf_off, b->tx_leaf_off[0], b->tx_leaf_off[b->ntx], b->leaf_bytes_len)) return false;
  if (!csr_ok(par, b->tx_tok_off, 0, b->ntx, b->ntok)) return false;
  std::atomic<bool> ok{true};
  par(b->ntx, 1u << 16, [&](uint64_t x, uint64_t y) {
    for (uint64_t t = x; t < y; t++) {
      uint64_t need;
      if (!pmt::slot_bound(b->tx_leaf_off[t + 1] - b->tx_leaf_off[t], &need) ||
          b->tx_tok_off[t + 1] - b->tx_tok_off[t] < need) {
        ok.store(false, std::memory_order_relaxed);
        return;
      }
    }
  });
  return ok.load();
}

// a signing batch: msg_off[0..n] non-decreasing and within msg_bytes, and no
// single message of 2^32 bytes or more (the kernel's message lengths are 32-bit).
// B: cordahip_sign_batch or cordahip_ecdsa_sign_batch (the same message fields).
template <class Par, class B>
bool check_sign_batch(Par&& par, const B* b) {
  if (b->n == 0) return true;
  if (!b->msg_off || !csr_ok(par, b->msg_off, 0, b->n, b->msg_bytes)) return false;
  std::atomic<bool> ok{true};
  par(b->n, 1u << 16, [&](uint64_t x, uint64_t y) {
    for (uint64_t i = x; i < y; i++)
      if (b->msg_off[i + 1] - b->msg_off[i] > 0xffffffffull) {
        ok.store(false, std::memory_order_relaxed);
        return;
      }
  });
  return ok.load();
}

// a keyed verification batch: sig_off[0..n] and msg_off[0..n] non-decreasing and
// within sig_bytes / msg_bytes, and no single message of 2^32 bytes or more (the
// kernel's message lengths are 32-bit; a signature of any length is a status)
template <class Par>
bool check_keyed_sig_batch(Par&& par, const cordahip_keyed_sig_batch* b) {
  if (b->n == 0) return true;
  if (!b->sig_off || !csr_ok(par, b->sig_off, 0, b->n, b->sig_bytes)) return false;
  if (!b->msg_off || !csr_ok(par, b->msg_off, 0, b->n, b->msg_bytes)) return false;
  std::atomic<bool> ok{true};
  par(b->n, 1u << 16, [&](uint64_t x, uint64_t y) {
    for (uint64_t i = x; i < y; i++)
      if (b->msg_off[i + 1] - b->msg_off[i] > 0xffffffffull) {
        ok.store(false, std::memory_order_relaxed);
        return;
      }
  });
  return ok.load();
}

// a commit batch (notary commit log): |now_ns| < 2^61 and 0 <= tolerance_ns < 2^61
// (the time-window differences then cannot overflow), tw_from and tw_until both
// given or both null, tx_ref_off[0..ntx] non-decreasing and within n_refs
template <class Par>
bool check_commit(Par&& par, const cordahip_commit_batch* b) {
  const int64_t lim = (int64_t)1 << 61;
  if (b->now_ns <= -lim || b->now_ns >= lim || b->tolerance_ns < 0 || b->tolerance_ns >= lim) return false;
  if ((b->tw_from == nullptr) != (b->tw_until == nullptr)) return false;
  if (b->ntx == 0) return true;
  return b->tx_ref_off && csr_ok(par, b->tx_ref_off, 0, b->ntx, b->n_refs);
}

// a typed notary tear-off batch: the window arrays all given or all null,
// tx_ref_off[0..ntx] non-decreasing and within n_refs, tx_tok_off[0..ntx]
// non-decreasing and within ntok (both whole, whatever a shard will read)
template <class Par>
bool check_notary_tearoff(Par&& par, const cordahip_notary_tearoff_batch* b) {
  const int given = (b->tw_flags != nullptr) + (b->tw_from_s != nullptr) + (b->tw_from_nano != nullptr) +
                    (b->tw_until_s != nullptr) + (b->tw_until_nano != nullptr);
  if (given != 0 && given != 5) return false;
  if (b->ntx == 0) return true;
  if (!b->tx_ref_off || !b->tx_tok_off) return false;
  return csr_ok(par, b->tx_ref_off, 0, b->ntx, b->n_refs) && csr_ok(par, b->tx_tok_off, 0, b->ntx, b->ntok);
}

// a cover (required-signer coverage): tx_req_off[0..ntx] non-decreasing and
// within nreq, req_tok_off over the required keys it spans within ntok, the
// whole key table's ckey_off[0..nckey] within ckey_bytes (any leaf may name any
// entry). Token contents are data: cover_core.hpp judges them per required key.
template <class Par>
bool check_cover(Par&& par, const cordahip_cover* c, uint64_t ntx) {
  if (ntx == 0) return true;
  if (!c->tx_req_off || !c->first_missing) return false;
  if (!csr_ok(par, c->tx_req_off, 0, ntx, c->nreq)) return false;
  const uint64_t r0 = c->tx_req_off[0], r1 = c->tx_req_off[ntx];
  if (r0 == r1) return true;  // no required keys: nothing else is read
  if (!c->req_status || !c->req_tok_off || !csr_ok(par, c->req_tok_off, r0, r1, c->ntok)) return false;
  if (c->req_tok_off[r0] != c->req_tok_off[r1] && !c->tok) return false;
  if (c->nckey == 0) return true;  // every leaf is malformed; the table is not read
  if (!c->ckey_scheme || !c->ckey_off || (c->ckey_bytes && !c->ckey)) return false;
  return csr_ok(par, c->ckey_off, 0, c->nckey, c->ckey_bytes);
}

}  // namespace rt
}  // namespace cordahip
