// The notary commit log's core (K16): slot layout, keyed slot index, probing, the
// time-window rule, one transaction's in-order commit and its report. Plain C++ for
// host and device: commit_log.hip runs it on the GPU, tools/commit_core_check.cpp
// and tools/commit_csr_fuzz.cpp run the same code under ASan/UBSan on the CPU.
//
// Restates, per transaction and in batch order,
//   TrustedAuthorityNotaryService.validateTimeWindow   NotaryService.kt:44-47
//     -> TimeWindowChecker.isValid                     TimeWindowChecker.kt:14-25
//   TrustedAuthorityNotaryService.commitInputStates    NotaryService.kt:53-67
//     -> PersistentUniquenessProvider.commit           PersistentUniquenessProvider.kt:62-82
// (model: tests/commit_log_model.py).
//
// Table: open addressing, linear probing, a power-of-two number of 96-byte slots:
//   words 0-1   state = the entry's sequence number + 1 (little-endian pair), 0 = empty
//   words 2-10  the StateRef (txhash[32], index)
//   words 11-20 the ConsumingTx (id[32], input_index, caller)
//   words 21-23 padding (word 21: the revoke mark, nonzero only between the two
//               launches of one cordahip_commit_log_revoke)
// An entry's key never changes, and an entry is removed only by
// cordahip_commit_log_revoke (erase_at / erase_row below): backward-shift deletion, which
// leaves the table as if the entry had never been put -- no tombstones, so every slot
// between an entry's home and its slot stays occupied and a probe still ends at the key
// or at the first empty slot. That is why find, put, insert_absent, the commit / load /
// lookup / rehash kernels, the host's bound and the visibility rule below are the same
// with removal as without it. The sequence number of transaction t of a batch is
// base + t (base: the log's running transaction counter, >= 1; loaded rows carry 0):
// a reader that belongs to transaction t sees an entry iff its sequence number is
// below t's, i.e. state <= base + t -- the log as it stood when the serial provider
// reached t, whatever later transactions of the batch have inserted since.
// The slot index is SipHash-1-3 of the 36 ref bytes under the log's 128-bit salt:
// ref bytes are chosen by clients, and only the probe length depends on the mix.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define COMMIT_HD __host__ __device__ inline
#else
#define COMMIT_HD inline
#endif

namespace cordahip {
namespace commit {

constexpr uint32_t kSlotWords = 24, kRefWords = 9, kByWords = 10;
constexpr uint32_t kSlotRef = 2, kSlotBy = 11, kSlotMark = 21;
constexpr uint8_t kRefAbsent = 0, kRefSelf = 1, kRefOther = 2;
// tx_status values (include/cordahip.h CORDAHIP_COMMIT_*)
constexpr uint8_t kCommitOk = 0, kCommitConflict = 16, kCommitTimeWindowInvalid = 17, kCommitSkipped = 18;
// a transaction's decision (one scratch byte per transaction of a call)
constexpr uint8_t kUndecided = 0, kCommits = 1, kReports = 2, kSkipped = 3, kWindowInvalid = 4;
constexpr int64_t kSideAbsent = INT64_MIN;
constexpr int64_t kSideBound = (int64_t)1 << 62;  // window sides are saturated here
constexpr uint64_t kNoFilter = ~0ull;

struct Table {
  uint32_t* slots;
  uint64_t mask;  // capacity - 1
  uint64_t k0, k1;
};

// the arrays of one call (cordahip_commit_batch); rows as 32-bit words
struct Batch {
  uint64_t ntx;
  const uint32_t* txid;    // 8 words per transaction
  const uint32_t* caller;
  const uint32_t* refs;    // kRefWords per input
  const uint64_t* off;     // [ntx + 1]
  const int64_t* tw_from;  // both null: no windows
  const int64_t* tw_until;
  int64_t now_ns, tolerance_ns;
  const uint8_t* gate;
  uint8_t* tx_status;
  uint8_t* committed;
  uint8_t* ref_state;
  uint32_t* ref_by;  // kByWords per input
};

COMMIT_HD uint64_t rotl64(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

#define COMMIT_SIPROUND        \
  do {                         \
    v0 += v1;                  \
    v1 = rotl64(v1, 13) ^ v0;  \
    v0 = rotl64(v0, 32);       \
    v2 += v3;                  \
    v3 = rotl64(v3, 16) ^ v2;  \
    v0 += v3;                  \
    v3 = rotl64(v3, 21) ^ v0;  \
    v2 += v1;                  \
    v1 = rotl64(v1, 17) ^ v2;  \
    v2 = rotl64(v2, 32);       \
  } while (0)

// SipHash-1-3 of the 36 bytes of a ref (words little-endian, as they lie in memory)
COMMIT_HD uint64_t hash_ref(const uint32_t* ref, uint64_t k0, uint64_t k1) {
  uint64_t v0 = k0 ^ 0x736f6d6570736575ull, v1 = k1 ^ 0x646f72616e646f6dull;
  uint64_t v2 = k0 ^ 0x6c7967656e657261ull, v3 = k1 ^ 0x7465646279746573ull;
  for (int i = 0; i < 4; i++) {
    const uint64_t m = (uint64_t)ref[2 * i] | ((uint64_t)ref[2 * i + 1] << 32);
    v3 ^= m;
    COMMIT_SIPROUND;
    v0 ^= m;
  }
  const uint64_t last = (uint64_t)ref[8] | (36ull << 56);
  v3 ^= last;
  COMMIT_SIPROUND;
  v0 ^= last;
  v2 ^= 0xff;
  COMMIT_SIPROUND;
  COMMIT_SIPROUND;
  COMMIT_SIPROUND;
  return v0 ^ v1 ^ v2 ^ v3;
}

COMMIT_HD uint64_t slot_state(const Table& T, uint64_t s) {
  const uint32_t* w = T.slots + s * kSlotWords;
  return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
}

COMMIT_HD bool ref_equal(const uint32_t* a, const uint32_t* b) {
  uint32_t d = 0;
  for (uint32_t i = 0; i < kRefWords; i++) d |= a[i] ^ b[i];
  return d == 0;
}

// The slot holding `ref` among the entries with state <= limit, or -1. The probe
// visits at most every slot once (a table kept below 7/8 load ends it far sooner).
COMMIT_HD int64_t find(const Table& T, const uint32_t* ref, uint64_t limit) {
  uint64_t s = hash_ref(ref, T.k0, T.k1) & T.mask;
  for (uint64_t n = 0; n <= T.mask; n++, s = (s + 1) & T.mask) {
    const uint64_t st = slot_state(T, s);
    if (st == 0) return -1;
    if (ref_equal(T.slots + s * kSlotWords + kSlotRef, ref)) return st <= limit ? (int64_t)s : -1;
  }
  return -1;
}

// ref -> by with the given state: a new entry (returns 1), or the entry of the same
// ref rewritten (returns 0: a transaction that lists a ref twice keeps the last
// position; a loaded row never takes this path, see load_row). -1: no free slot.
COMMIT_HD int put(const Table& T, const uint32_t* ref, uint64_t state, const uint32_t* by) {
  uint64_t s = hash_ref(ref, T.k0, T.k1) & T.mask;
  for (uint64_t n = 0; n <= T.mask; n++, s = (s + 1) & T.mask) {
    uint32_t* w = T.slots + s * kSlotWords;
    const uint64_t st = slot_state(T, s);
    const bool fresh = st == 0;
    if (!fresh && !ref_equal(w + kSlotRef, ref)) continue;
    for (uint32_t i = 0; i < kByWords; i++) w[kSlotBy + i] = by[i];
    if (fresh) {
      for (uint32_t i = 0; i < kRefWords; i++) w[kSlotRef + i] = ref[i];
      w[0] = (uint32_t)state;
      w[1] = (uint32_t)(state >> 32);
    }
    return fresh ? 1 : 0;
  }
  return -1;
}

// One row of cordahip_commit_log_load, rows taken in order: inserted with sequence
// number 0 unless its ref is there already (returns 0, the entry left alone). The
// kernels' claim + insert gives the same table; this is its in-order statement.
COMMIT_HD int load_row(const Table& T, const uint32_t* row) {
  if (find(T, row, kNoFilter) >= 0) return 0;
  return put(T, row, 1, row + kRefWords);
}

// The entry in slot i removed by backward shift: j walks forward from i to the first
// empty slot; an entry at j whose home slot lies cyclically in (i, j] stays, any other
// moves to i whole (state and padding included) and i becomes j; the last i is cleared
// whole. Entries move only backwards, inside the run of occupied slots that held i.
COMMIT_HD void erase_at(const Table& T, uint64_t i) {
  uint64_t j = i;
  for (uint64_t n = 0; n <= T.mask; n++) {
    j = (j + 1) & T.mask;
    if (slot_state(T, j) == 0) break;
    const uint32_t* src = T.slots + j * kSlotWords;
    const uint64_t home = hash_ref(src + kSlotRef, T.k0, T.k1) & T.mask;
    if (((j - home) & T.mask) < ((j - i) & T.mask)) continue;  // home in (i, j]
    uint32_t* dst = T.slots + i * kSlotWords;
    for (uint32_t q = 0; q < kSlotWords; q++) dst[q] = src[q];
    i = j;
  }
  uint32_t* w = T.slots + i * kSlotWords;
  for (uint32_t q = 0; q < kSlotWords; q++) w[q] = 0;
}

// the 40 bytes stored in slot s equal `by`
COMMIT_HD bool by_equal(const Table& T, uint64_t s, const uint32_t* by) {
  const uint32_t* w = T.slots + s * kSlotWords + kSlotBy;
  uint32_t d = 0;
  for (uint32_t q = 0; q < kByWords; q++) d |= w[q] ^ by[q];
  return d == 0;
}

// One row of cordahip_commit_log_revoke, rows taken in order: the entry of the row's
// ref removed iff its stored ConsumingTx equals the row's in all 40 bytes (returns 1),
// else nothing touched (returns 0). The kernels' mark + repair gives the same table;
// this is its in-order statement.
COMMIT_HD int erase_row(const Table& T, const uint32_t* row) {
  const int64_t s = find(T, row, kNoFilter);
  if (s < 0 || !by_equal(T, (uint64_t)s, row + kRefWords)) return 0;
  erase_at(T, (uint64_t)s);
  return 1;
}

// The repair of one cluster (a maximal cyclic run of occupied slots) that begins at
// `start` (its predecessor is empty): every entry whose mark word is set is removed.
// The cluster is measured first, then its original extent walked: erase_at at a marked
// slot and the same position looked at again (a marked entry may have moved in), else
// one step on, over the holes earlier shifts opened. Shifts stay inside the extent and
// never write a slot that was empty when the walk began, so clusters are independent.
// Returns the entries removed.
COMMIT_HD uint64_t repair_cluster(const Table& T, uint64_t start) {
  uint64_t len = 0;
  while (len <= T.mask && slot_state(T, (start + len) & T.mask) != 0) len++;
  uint64_t removed = 0;
  for (uint64_t p = 0; p < len;) {
    const uint64_t s = (start + p) & T.mask;
    if (slot_state(T, s) != 0 && T.slots[s * kSlotWords + kSlotMark] != 0) {
      erase_at(T, s);  // one entry fewer each time: at most len times in all
      removed++;
    } else {
      p++;
    }
  }
  return removed;
}

// TimeWindowChecker.isValid (:22-23), exact in nanoseconds. The caller saturates
// from / until at +-2^62 (a side beyond that is cut there again here, which changes no
// verdict: |now| + tolerance < 2^62) and |now| < 2^61: neither difference overflows.
COMMIT_HD int64_t saturate_side(int64_t v) { return v > kSideBound ? kSideBound : v < -kSideBound ? -kSideBound : v; }
COMMIT_HD bool window_valid(int64_t from, int64_t until, int64_t now, int64_t tol) {
  if (until != kSideAbsent && now - saturate_side(until) > tol) return false;
  if (from != kSideAbsent && saturate_side(from) - now > tol) return false;
  return true;
}

COMMIT_HD void zero_rows(const Batch& B, uint64_t t) {
  for (uint64_t i = B.off[t]; i < B.off[t + 1]; i++) {
    B.ref_state[i] = kRefAbsent;
    for (uint32_t q = 0; q < kByWords; q++) B.ref_by[i * kByWords + q] = 0;
  }
}

// Gate and time window of transaction t: kSkipped / kWindowInvalid with the status,
// the committed byte and zero rows written, or kUndecided with nothing written.
COMMIT_HD uint8_t gate_and_window(const Batch& B, uint64_t t) {
  uint8_t d = kUndecided;
  if (B.gate && B.gate[t]) d = kSkipped;
  else if (B.tw_from && !window_valid(B.tw_from[t], B.tw_until[t], B.now_ns, B.tolerance_ns)) d = kWindowInvalid;
  if (d == kUndecided) return d;
  B.tx_status[t] = d == kSkipped ? kCommitSkipped : kCommitTimeWindowInvalid;
  B.committed[t] = 0;
  zero_rows(B, t);
  return d;
}

// some input of transaction t is in the log as transaction t sees it
COMMIT_HD bool any_present(const Table& T, const Batch& B, uint64_t t, uint64_t limit) {
  for (uint64_t i = B.off[t]; i < B.off[t + 1]; i++)
    if (find(T, B.refs + i * kRefWords, limit) >= 0) return true;
  return false;
}

// PersistentUniquenessProvider.commit for transaction t, in order: nothing present
// -> every input put in list order (kCommits, *added += the new entries), else
// kReports with the log untouched.
COMMIT_HD uint8_t commit_tx(const Table& T, const Batch& B, uint64_t t, uint64_t base, uint64_t* added) {
  if (any_present(T, B, t, base + t)) return kReports;
  uint32_t by[kByWords];
  for (uint32_t q = 0; q < 8; q++) by[q] = B.txid[t * 8 + q];
  by[9] = B.caller[t];
  for (uint64_t i = B.off[t]; i < B.off[t + 1]; i++) {
    by[8] = (uint32_t)(i - B.off[t]);
    if (put(T, B.refs + i * kRefWords, base + t + 1, by) == 1) (*added)++;
  }
  return kCommits;
}

// The outputs of a transaction that passed gate and window. d == kCommits: OK,
// committed, zero rows. d == kReports: every input looked up as transaction t sees
// the log; OK (already committed: every present input stores exactly this id,
// position and caller) or COMMIT_CONFLICT.
COMMIT_HD void report_tx(const Table& T, const Batch& B, uint64_t t, uint64_t base, uint8_t d) {
  if (d == kCommits) {
    B.tx_status[t] = kCommitOk;
    B.committed[t] = 1;
    zero_rows(B, t);
    return;
  }
  bool other = false;
  for (uint64_t i = B.off[t]; i < B.off[t + 1]; i++) {
    const int64_t s = find(T, B.refs + i * kRefWords, base + t);
    uint32_t* by = B.ref_by + i * kByWords;
    if (s < 0) {
      B.ref_state[i] = kRefAbsent;
      for (uint32_t q = 0; q < kByWords; q++) by[q] = 0;
      continue;
    }
    const uint32_t* w = T.slots + (uint64_t)s * kSlotWords + kSlotBy;
    uint32_t diff = (w[8] ^ (uint32_t)(i - B.off[t])) | (w[9] ^ B.caller[t]);
    for (uint32_t q = 0; q < 8; q++) diff |= w[q] ^ B.txid[t * 8 + q];
    for (uint32_t q = 0; q < kByWords; q++) by[q] = w[q];
    B.ref_state[i] = diff ? kRefOther : kRefSelf;
    other |= diff != 0;
  }
  B.tx_status[t] = other ? kCommitConflict : kCommitOk;
  B.committed[t] = 0;
}

// A whole batch one transaction at a time (the in-order sweep with nothing decided
// before it, and the host check tool's path). Returns the entries added.
COMMIT_HD uint64_t run_serial(const Table& T, const Batch& B, uint64_t base) {
  uint64_t added = 0;
  for (uint64_t t = 0; t < B.ntx; t++) {
    if (gate_and_window(B, t) != kUndecided) continue;
    report_tx(T, B, t, base, commit_tx(T, B, t, base, &added));
  }
  return added;
}

}  // namespace commit
}  // namespace cordahip
