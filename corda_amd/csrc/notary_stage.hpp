// The host side of a batch of typed notary tear-offs (cordahip_notary_tearoff_*): the
// layout of transactions [t0, t1) in one stage buffer -- inputs, outputs, then scratch that
// only the device image has, every array at a 16-byte boundary -- the copy of the caller's
// arrays into its host image, and the K21 + K6 enqueue over its device image. Shared by
// the verify shards (cordahip.cpp) and the commit call (commit_api.cpp), which appends
// K16's arrays ahead of the scratch.
// The batch's CSR arrays have been checked (csr_check.hpp check_notary_tearoff).
#pragma once
#include <cstring>

#include "runtime.hpp"

#pragma GCC visibility push(hidden)
namespace cordahip {
namespace rt {

struct NotaryStage {
  uint64_t t0, ntx, r0, nr, k0, ntok;
  bool win;
  size_t pos = 0;
  // inputs [0, in_bytes)
  size_t o_refs, o_off, o_koff, o_root, o_tok, o_tokh, o_flags, o_fs, o_us, o_fn, o_un, in_bytes;
  // outputs [o_vst, out_end): verify statuses, leaf hashes (bytes)
  size_t o_vst, o_lh, out_end;
  // device only: tx_leaf_off, bad, the windows in ns, leaf hashes as K6's words, K6's stack
  size_t host_bytes = 0, o_loff = 0, o_bad = 0, o_twf = 0, o_twu = 0, o_hashes = 0, o_stack = 0;

  size_t take(size_t bytes) {
    const size_t at = pos;
    pos = (pos + bytes + 15) & ~(size_t)15;
    return at;
  }
  NotaryStage(const cordahip_notary_tearoff_batch* b, uint64_t t0_, uint64_t t1) : t0(t0_), ntx(t1 - t0_) {
    r0 = b->tx_ref_off[t0], nr = b->tx_ref_off[t1] - r0;
    k0 = b->tx_tok_off[t0], ntok = b->tx_tok_off[t1] - k0;
    win = b->tw_flags != nullptr;
    o_refs = take(nr * sizeof(cordahip_state_ref));
    o_off = take((ntx + 1) * 8);
    o_koff = take((ntx + 1) * 8);
    o_root = take(ntx * 32);
    o_tok = take(ntok);
    o_tokh = take(ntok * 32);
    o_flags = take(win ? ntx : 0);
    o_fs = take(win ? ntx * 8 : 0);
    o_us = take(win ? ntx * 8 : 0);
    o_fn = take(win ? ntx * 4 : 0);
    o_un = take(win ? ntx * 4 : 0);
    in_bytes = pos;
    o_vst = take(ntx);
    o_lh = take((nr + ntx) * 32);
    out_end = pos;
  }
  // the device-only arrays, behind everything the host image holds (call last)
  void scratch() {
    host_bytes = pos;
    o_loff = take((ntx + 1) * 8);
    o_bad = take(ntx);
    o_twf = take(ntx * 8);
    o_twu = take(ntx * 8);
    o_hashes = take((nr + ntx) * 32);
    o_stack = take((ntok ? ntok : 1) * 32);
  }
  // the caller's arrays into the host image h (at least in_bytes)
  void fill(const cordahip_notary_tearoff_batch* b, uint8_t* h) const {
    if (nr) std::memcpy(h + o_refs, b->refs + r0, nr * sizeof(cordahip_state_ref));
    uint64_t* off = reinterpret_cast<uint64_t*>(h + o_off);
    uint64_t* koff = reinterpret_cast<uint64_t*>(h + o_koff);
    for (uint64_t t = 0; t <= ntx; t++) {
      off[t] = b->tx_ref_off[t0 + t] - r0;
      koff[t] = b->tx_tok_off[t0 + t] - k0;
    }
    std::memcpy(h + o_root, b->root + t0 * 32, ntx * 32);
    if (ntok) {
      std::memcpy(h + o_tok, b->tok + k0, ntok);
      std::memcpy(h + o_tokh, b->tok_hash + k0 * 32, ntok * 32);
    }
    if (win) {
      std::memcpy(h + o_flags, b->tw_flags + t0, ntx);
      std::memcpy(h + o_fs, b->tw_from_s + t0, ntx * 8);
      std::memcpy(h + o_us, b->tw_until_s + t0, ntx * 8);
      std::memcpy(h + o_fn, b->tw_from_nano + t0, ntx * 4);
      std::memcpy(h + o_un, b->tw_until_nano + t0, ntx * 4);
    }
  }
  NotaryRows rows(const uint8_t* dv) const {
    NotaryRows R{};
    R.ntx = ntx, R.n_refs = nr;
    R.refs = reinterpret_cast<const cordahip_state_ref*>(dv + o_refs);
    R.tx_ref_off = reinterpret_cast<const uint64_t*>(dv + o_off);
    if (win) {
      R.tw_flags = dv + o_flags;
      R.tw_from_s = reinterpret_cast<const int64_t*>(dv + o_fs);
      R.tw_until_s = reinterpret_cast<const int64_t*>(dv + o_us);
      R.tw_from_nano = reinterpret_cast<const int32_t*>(dv + o_fn);
      R.tw_until_nano = reinterpret_cast<const int32_t*>(dv + o_un);
    }
    return R;
  }
  // K21, then K6: the verify statuses at o_vst, the windows at o_twf / o_twu
  hipError_t enqueue_verify(uint8_t* dv, bool leaf_hash, hipStream_t s) const {
    uint64_t* loff = reinterpret_cast<uint64_t*>(dv + o_loff);
    uint32_t* hashes = reinterpret_cast<uint32_t*>(dv + o_hashes);
    hipError_t e = launch_notary_leaves(rows(dv), loff, hashes, leaf_hash ? dv + o_lh : nullptr,
                                        reinterpret_cast<int64_t*>(dv + o_twf), reinterpret_cast<int64_t*>(dv + o_twu),
                                        dv + o_bad, s);
    return e ? e
             : launch_pmt_verify(hashes, loff, dv + o_tok, dv + o_tokh, reinterpret_cast<const uint64_t*>(dv + o_koff),
                                 dv + o_root, ntx, reinterpret_cast<uint32_t*>(dv + o_stack), dv + o_vst, s, dv + o_bad);
  }
  // the leaves of [t0, t1) in the caller's leaf_hash: its refs and windows before t0
  static uint64_t leaves_before(const cordahip_notary_tearoff_batch* b, uint64_t t) {
    uint64_t n = b->tx_ref_off[t] - b->tx_ref_off[0];
    if (b->tw_flags)
      for (uint64_t i = 0; i < t; i++) n += (b->tw_flags[i] >> 7) & 1;
    return n;
  }
};

// the pointers a typed tear-off batch must carry (host forms, after the CSR check)
inline bool notary_pointers_ok(const cordahip_notary_tearoff_batch* b) {
  const uint64_t n = b->ntx;
  if (!b->root || !b->tx_status) return false;
  if (b->tx_ref_off[n] != b->tx_ref_off[0] && !b->refs) return false;
  if (b->tx_tok_off[n] != b->tx_tok_off[0] && (!b->tok || !b->tok_hash)) return false;
  return true;
}

}  // namespace rt
}  // namespace cordahip
#pragma GCC visibility pop
