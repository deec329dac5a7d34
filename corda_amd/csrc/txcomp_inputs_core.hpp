// A full transaction's inputs and time window out of its component items (K22): the
// per-transaction rule of cordahip_txcomp_inputs_device. Plain C++ for host and device:
// txcomp_inputs.hip runs it on the GPU, tools/txcomp_inputs_check.cpp runs the same code
// under ASan/UBSan on the CPU (model: tests/kryo_payment_model.py extract_inputs).
//
// The items are those of a cordahip_signed_txcomp_verify_ed25519_device batch: `data` is
// an OFFSET into the payload. A transaction's inputs are its STATE_REF items in item
// order, its window its one TIME_WINDOW item; every other kind is skipped. Three steps,
// one kernel each:
//   scan_tx   a transaction's items: validate, count the refs, derive the window
//   place     the exclusive scan's running count -> the clamped offset and the gate
//   copy_tx   the refs, as 36-byte rows, to where place put them
// Nothing here trusts an offset: an item range is cut to n_items, a payload range is
// checked against payload_len before it is read, and copy_tx writes rows only below the
// clamped end that place derived from ref_cap.
#pragma once
#include <stdint.h>

#include "kryo_core.hpp"

namespace cordahip {
namespace txin {

constexpr int64_t kAbsent = INT64_MIN;
constexpr uint8_t kBadComponent = 9;  // CORDAHIP_TX_BAD_COMPONENT
constexpr uint32_t kRefWords = kryo::kStateRefLen / 4;

// an Instant as cordahip_commit_batch's bounds: ns since the epoch, saturated at +-2^62
// (|s| <= 4611686019: the product and the sum stay inside int64)
KRYO_HD inline int64_t instant_ns(int64_t s, int32_t nano) {
  const int64_t lim = (int64_t)1 << 62;
  if (s > 4611686018ll) return lim;
  if (s < -4611686019ll) return -lim;
  const int64_t v = s * 1000000000ll + nano;
  return v > lim ? lim : v < -lim ? -lim : v;
}

struct Batch {
  const cordahip_kryo_item* items;
  uint64_t n_items;
  const uint8_t* payload;
  uint64_t payload_len;
  const uint64_t* tx_item_off;  // [ntx + 1], untrusted
  uint64_t ntx;
};

// transaction t's items [i0, i1), cut to n_items; a reversed range is empty
KRYO_HD inline void item_range(const Batch& b, uint64_t t, uint64_t& i0, uint64_t& i1) {
  const uint64_t a = b.tx_item_off[t], e = b.tx_item_off[t + 1];
  i0 = a < b.n_items ? a : b.n_items;
  i1 = e < b.n_items ? e : b.n_items;
  if (i1 < i0) i1 = i0;
}

// the item's payload, or nullptr when it is not `len` bytes wholly inside the payload
KRYO_HD inline const uint8_t* payload_of(const Batch& b, const cordahip_kryo_item& it, uint64_t len) {
  const uint64_t off = (uint64_t)(uintptr_t)it.data;
  if (it.len != len || off > b.payload_len || len > b.payload_len - off) return nullptr;
  return b.payload + off;
}

struct TxScan {
  uint64_t nref = 0;  // 0 when flagged
  int64_t tw_from = kAbsent, tw_until = kAbsent;
  bool flagged = false;
};

KRYO_HD inline TxScan scan_tx(const Batch& b, uint64_t t) {
  uint64_t i0, i1;
  item_range(b, t, i0, i1);
  TxScan x;
  uint32_t windows = 0;
  for (uint64_t i = i0; i < i1; i++) {
    const uint32_t kind = b.items[i].kind;
    if (kind == CORDAHIP_KRYO_STATE_REF) {
      if (payload_of(b, b.items[i], kryo::kStateRefLen)) x.nref++;
      else x.flagged = true;
    } else if (kind == CORDAHIP_KRYO_TIME_WINDOW) {
      cordahip_kryo_item it = b.items[i];
      it.data = payload_of(b, it, kryo::kTimeWindowLen);
      const kryo::TimeWindowRow r = kryo::time_window_row(it);  // a missing payload: not ok
      if (!r.ok || ++windows > 1) {
        x.flagged = true;
      } else {
        if (r.flags & 1u) x.tw_from = instant_ns(r.s[0], r.n[0]);
        if (r.flags & 2u) x.tw_until = instant_ns(r.s[1], r.n[1]);
      }
    }
  }
  if (x.flagged) x.nref = 0, x.tw_from = x.tw_until = kAbsent;
  return x;
}

KRYO_HD inline uint64_t add_sat(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// A transaction whose refs are [start, start + nref) before clamping: its offset, and
// its gate byte (status: d_tx_status[t], 0 when not given).
KRYO_HD inline uint64_t place(uint64_t start, uint64_t nref, bool flagged, uint64_t ref_cap, uint8_t status,
                              uint8_t& gate) {
  if (add_sat(start, nref) > ref_cap) flagged = true;
  gate = status ? status : flagged ? kBadComponent : 0;
  return start < ref_cap ? start : ref_cap;
}

// 36 bytes from src (any alignment) to the 4-byte aligned row dst
KRYO_HD inline void copy_ref(const uint8_t* src, uint32_t* dst) {
#if defined(__HIP_DEVICE_COMPILE__)
  // aligned dword loads, each holding a wanted byte (so all are mapped), and a funnel shift
  const uintptr_t a = (uintptr_t)src & ~(uintptr_t)3;
  const uint32_t sb = (uint32_t)((uintptr_t)src & 3);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a);
  uint32_t w[kRefWords + 1];
#pragma unroll
  for (uint32_t i = 0; i < kRefWords; i++) w[i] = q[i];
  w[kRefWords] = sb ? q[kRefWords] : 0;
#pragma unroll
  for (uint32_t i = 0; i < kRefWords; i++) dst[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sb);
#else
  for (uint32_t i = 0; i < kRefWords; i++) dst[i] = kryo::le32(src + 4 * i);
#endif
}

// Transaction t's first `rows` refs to dst (rows of kRefWords words). rows = the clamped
// range's length: at most scan_tx's nref, so a flagged transaction copies nothing.
KRYO_HD inline void copy_tx(const Batch& b, uint64_t t, uint32_t* dst, uint64_t rows) {
  uint64_t i0, i1;
  item_range(b, t, i0, i1);
  uint64_t k = 0;
  for (uint64_t i = i0; i < i1 && k < rows; i++) {
    if (b.items[i].kind != CORDAHIP_KRYO_STATE_REF) continue;
    const uint8_t* src = payload_of(b, b.items[i], kryo::kStateRefLen);
    if (!src) continue;
    copy_ref(src, dst + k * kRefWords);
    k++;
  }
}

}  // namespace txin
}  // namespace cordahip
