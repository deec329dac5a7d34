// The notary commit log on the GPU -- kernel K16 (gfx950).
//
// Replaces, per batch of notarisation requests, the serial loop of
//   TrustedAuthorityNotaryService.validateTimeWindow / commitInputStates
//     (NotaryService.kt:44-47, :53-67)
//   -> PersistentUniquenessProvider.commit (PersistentUniquenessProvider.kt:62-82)
// over a device-resident table of consumed StateRefs (commit_core.hpp: layout,
// keyed slot index, the per-transaction routines shared with the host check tools).
//
// A call is a chain of launches on one stream; the kernel boundaries are the only
// fences:
//   clamp    the offsets copied with every entry cut to n_refs, so no later kernel
//            indexes outside the caller's arrays whatever the device arrays hold
//   pre-pass one lane per transaction: gate, time window, and a lookup of every
//            input in the log as it stood before the batch; a transaction with a
//            present input is decided (it reports), a skipped or out-of-window one
//            is finished; the rest are counted in a device-side "undecided" word
//   rounds   R times (CORDAHIP_COMMIT_ROUNDS, default 2, 0 allowed) claim / win /
//            lose, one lane per transaction:
//     claim  every input of every undecided transaction into a per-call scratch
//            table of 64-bit input ordinals (at least 2 n_refs slots): an empty
//            slot is taken by compare-and-swap, a slot whose ordinal names an
//            equal ref takes atomicMin -- equality is tested against the
//            immutable input array -- so each distinct ref ends up holding the
//            smallest ordinal that claims it
//     win    a transaction whose every input holds an ordinal of its own commits:
//            no earlier undecided transaction touches its refs, and none can have
//            been consumed under a smaller sequence number (pre-pass, lose). The
//            first occurrence of each distinct ref inserts it with the
//            transaction's sequence number and the ref's LAST position. No key is
//            compared: a winner's refs are in the log under no sequence number at
//            all (a later transaction that won an earlier round would have had to
//            own a ref this one was claiming with a smaller ordinal), and the keys
//            inserted by one launch are distinct, so any occupied slot is someone
//            else's and the probe claims the first empty one
//     lose   an undecided transaction with an input now in the log under a smaller
//            sequence number is decided (it reports)
//            Every launch returns at once when the undecided word is zero.
//   sweep    one lane takes what is still undecided in batch order (lookups
//            filtered by sequence number, then the puts): exact for every batch,
//            chains t_k ^ t_{k+1} != {} included, which defeat any round count
//   report   one lane per transaction: statuses, committed bytes, ref_state / ref_by
// cordahip_commit_log_load is claim + insert over its rows (each distinct new ref's first
// row inserts it), cordahip_commit_log_reserve a rehash with the same insert,
// cordahip_commit_log_revoke mark + repair (backward-shift deletion, one lane per
// cluster), cordahip_commit_log_export one pass over the slots.
// Visibility: within a launch lanes communicate only through 64-bit agent-scope
// atomics -- the claim table's ordinals, the state word of a log slot, the counters.
// Slot payloads are written with plain stores and read only by later launches. The
// pre-pass, lose and the report only read the table; the sweep is one lane reading
// its own stores; the rehash, like win, claims empty slots by compare-and-swap on
// the state word and looks at no payload (every key of the old table is distinct);
// the revoke's mark launch changes only mark words (atomicOr), and its repair launch
// is one lane per cluster reading its own stores.
// Oracle: tests/commit_log_model.py (tests/commit_revoke_model.py for revoke / export).
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>

#include "commit_core.hpp"

namespace cordahip {

using namespace commit;

constexpr unsigned long long kClaimEmpty = ~0ull;
static uint64_t claim_slots(uint64_t n_refs);

// v summed over the wave, one atomic per wave (every lane of the wave calls it)
__device__ inline void wave_add(unsigned long long* ctr, long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(ctr, (unsigned long long)v);
}

// Nothing is undecided (the word only ever falls during the rounds): one atomic read
// per wave, the same answer for all of its lanes. Called by every lane of the wave.
__device__ inline bool none_undecided(unsigned long long* undecided) {
  unsigned long long v = 0;
  if ((threadIdx.x & 63) == 0) v = atomicAdd(undecided, 0ull);
  return __shfl(v, 0, 64) == 0ull;
}

__global__ void __launch_bounds__(256) commit_clamp_kernel(const uint64_t* __restrict__ off, uint64_t n,
                                                           uint64_t n_refs, uint64_t* __restrict__ out,
                                                           unsigned long long* __restrict__ undecided) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *undecided = 0;
  if (i >= n) return;
  const uint64_t v = off[i];
  out[i] = v < n_refs ? v : n_refs;
}

__global__ void __launch_bounds__(256) commit_prepass_kernel(Table T, Batch B, uint64_t base,
                                                             uint8_t* __restrict__ decided,
                                                             unsigned long long* __restrict__ undecided) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint8_t d = kSkipped;
  if (t < B.ntx) {
    d = gate_and_window(B, t);
    if (d == kUndecided && any_present(T, B, t, base + t)) d = kReports;
    decided[t] = d;
  }
  wave_add(undecided, d == kUndecided);
}

// The claim table's slot for the ref of row i (rows of `stride` words that begin with
// a ref): the slot whose ordinal names an equal ref, or the first empty one (take:
// claimed with ordinal i). Returns the slot's ordinal after the visit (kClaimEmpty: not
// found and not taken). cmask + 1 is at least twice the number of rows.
__device__ inline unsigned long long claim_visit(unsigned long long* claim, uint64_t cmask, const uint32_t* rows,
                                                 uint32_t stride, const Table& T, uint64_t i, bool take) {
  const uint32_t* ref = rows + i * stride;
  uint64_t s = hash_ref(ref, T.k1, T.k0) & cmask;
  for (uint64_t n = 0; n <= cmask; n++, s = (s + 1) & cmask) {
    unsigned long long cur = atomicAdd(claim + s, 0ull);
    if (cur == kClaimEmpty) {
      if (!take) return kClaimEmpty;
      cur = atomicCAS(claim + s, kClaimEmpty, (unsigned long long)i);
      if (cur == kClaimEmpty) return i;
    }
    if (!ref_equal(rows + cur * stride, ref)) continue;
    if (!take) return cur;
    const unsigned long long old = atomicMin(claim + s, (unsigned long long)i);
    return old < i ? old : i;
  }
  return kClaimEmpty;
}

// A key that is in the log under no sequence number, and that no other lane of this
// launch inserts, into the first empty slot of its probe sequence: compare-and-swap
// on the state word, then the payload with plain stores (read by later launches
// only). No key is compared -- every occupied slot is someone else's.
__device__ inline bool insert_absent(const Table& T, const uint32_t* ref, uint64_t state, const uint32_t* id,
                                     uint32_t input_index, uint32_t caller) {
  uint64_t s = hash_ref(ref, T.k0, T.k1) & T.mask;
  for (uint64_t n = 0; n <= T.mask; n++, s = (s + 1) & T.mask) {
    uint32_t* w = T.slots + s * kSlotWords;
    if (atomicCAS(reinterpret_cast<unsigned long long*>(w), 0ull, (unsigned long long)state) != 0ull) continue;
    for (uint32_t q = 0; q < kRefWords; q++) w[kSlotRef + q] = ref[q];
    for (uint32_t q = 0; q < 8; q++) w[kSlotBy + q] = id[q];
    w[kSlotBy + 8] = input_index;
    w[kSlotBy + 9] = caller;
    return true;
  }
  return false;
}

__global__ void __launch_bounds__(256) commit_claim_kernel(Table T, Batch B, const uint8_t* __restrict__ decided,
                                                           unsigned long long* __restrict__ claim, uint64_t cmask,
                                                           unsigned long long* __restrict__ undecided) {
  if (none_undecided(undecided)) return;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B.ntx || decided[t] != kUndecided) return;
  for (uint64_t i = B.off[t]; i < B.off[t + 1]; i++) (void)claim_visit(claim, cmask, B.refs, kRefWords, T, i, true);
}

__global__ void __launch_bounds__(256) commit_win_kernel(Table T, Batch B, uint64_t base,
                                                         uint8_t* __restrict__ decided,
                                                         unsigned long long* __restrict__ claim, uint64_t cmask,
                                                         unsigned long long* __restrict__ undecided,
                                                         unsigned long long* __restrict__ entries) {
  if (none_undecided(undecided)) return;  // wave-uniform: the lanes that go on all reach the wave_adds below
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool wins = t < B.ntx && decided[t] == kUndecided;
  const uint64_t lo = wins ? B.off[t] : 0, hi = wins ? B.off[t + 1] : 0;
  for (uint64_t i = lo; i < hi && wins; i++) {
    const unsigned long long m = claim_visit(claim, cmask, B.refs, kRefWords, T, i, false);
    wins = m >= lo && m < hi;  // the smallest claimant of this ref is an input of this transaction
  }
  long long added = 0;
  if (wins) {
    decided[t] = kCommits;
    const uint64_t state = base + t + 1;
    for (uint64_t i = lo; i < hi; i++) {
      const uint32_t* ref = B.refs + i * kRefWords;
      uint64_t last = i;
      bool first = true;
      for (uint64_t j = lo; j < hi; j++) {
        if (j == i || !ref_equal(B.refs + j * kRefWords, ref)) continue;
        first &= j > i;
        last = j > last ? j : last;
      }
      if (!first) continue;  // an earlier position of this transaction inserts the ref
      added += insert_absent(T, ref, state, B.txid + t * 8, (uint32_t)(last - lo), B.caller[t]);
    }
  }
  wave_add(entries, added);
  wave_add(undecided, wins ? -1 : 0);
}

__global__ void __launch_bounds__(256) commit_lose_kernel(Table T, Batch B, uint64_t base,
                                                          uint8_t* __restrict__ decided,
                                                          unsigned long long* __restrict__ undecided) {
  if (none_undecided(undecided)) return;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool loses = t < B.ntx && decided[t] == kUndecided && any_present(T, B, t, base + t);
  if (loses) decided[t] = kReports;
  wave_add(undecided, loses ? -1 : 0);
}

__global__ void __launch_bounds__(64) commit_sweep_kernel(Table T, Batch B, uint64_t base,
                                                          uint8_t* __restrict__ decided,
                                                          unsigned long long* __restrict__ undecided,
                                                          unsigned long long* __restrict__ entries) {
  if (blockIdx.x || threadIdx.x || *undecided == 0) return;
  uint64_t added = 0;
  for (uint64_t t = 0; t < B.ntx; t++)
    if (decided[t] == kUndecided) decided[t] = commit_tx(T, B, t, base, &added);
  *entries += added;
}

__global__ void __launch_bounds__(256) commit_report_kernel(Table T, Batch B, uint64_t base,
                                                            const uint8_t* __restrict__ decided) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= B.ntx) return;
  const uint8_t d = decided[t];
  if (d == kCommits || d == kReports) report_tx(T, B, t, base, d);
}

// cordahip_commit_log_lookup: the report's probe with no filter
__global__ void __launch_bounds__(256) commit_lookup_kernel(Table T, const uint32_t* __restrict__ refs, uint64_t n,
                                                            uint8_t* __restrict__ present,
                                                            uint32_t* __restrict__ by) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t s = find(T, refs + i * kRefWords, kNoFilter);
  present[i] = s >= 0;
  const uint32_t* w = T.slots + (uint64_t)(s < 0 ? 0 : s) * kSlotWords + kSlotBy;
  for (uint32_t q = 0; q < kByWords; q++) by[i * kByWords + q] = s < 0 ? 0u : w[q];
}

// cordahip_commit_log_load, two launches, one lane per row. claim: a row whose ref the
// log holds already is marked; the others claim their ref in the scratch table, so each
// distinct new ref holds its first row. insert: that first row inserts the ref with
// sequence number 0; every other row counts in counters[1] (present already, or earlier
// in the call). counters[0] is the log's entry count.
__global__ void __launch_bounds__(256) commit_load_claim_kernel(Table T, const uint32_t* __restrict__ rows,
                                                                uint64_t n, unsigned long long* __restrict__ claim,
                                                                uint64_t cmask, uint8_t* __restrict__ fresh,
                                                                unsigned long long* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) counters[1] = 0;
  if (i >= n) return;
  const bool f = find(T, rows + i * (kRefWords + kByWords), kNoFilter) < 0;
  fresh[i] = f;
  if (f) (void)claim_visit(claim, cmask, rows, kRefWords + kByWords, T, i, true);
}

__global__ void __launch_bounds__(256) commit_load_insert_kernel(Table T, const uint32_t* __restrict__ rows,
                                                                 uint64_t n, unsigned long long* __restrict__ claim,
                                                                 uint64_t cmask, const uint8_t* __restrict__ fresh,
                                                                 unsigned long long* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool ins = false;
  if (i < n && fresh[i] && claim_visit(claim, cmask, rows, kRefWords + kByWords, T, i, false) == i) {
    const uint32_t* row = rows + i * (kRefWords + kByWords);
    ins = insert_absent(T, row, 1, row + kRefWords, row[kRefWords + 8], row[kRefWords + 9]);
  }
  wave_add(counters, ins);
  wave_add(counters + 1, i < n && !ins);
}

// cordahip_commit_log_reserve: every entry of the old table into the new, empty one
__global__ void __launch_bounds__(256) commit_rehash_kernel(Table from, Table to) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > from.mask) return;
  const uint64_t st = slot_state(from, i);
  if (st == 0) return;
  const uint32_t* src = from.slots + i * kSlotWords;
  uint64_t s = hash_ref(src + kSlotRef, to.k0, to.k1) & to.mask;
  for (uint64_t n = 0; n <= to.mask; n++, s = (s + 1) & to.mask) {
    uint32_t* dst = to.slots + s * kSlotWords;
    if (atomicCAS(reinterpret_cast<unsigned long long*>(dst), 0ull, (unsigned long long)st) != 0ull) continue;
    for (uint32_t q = 2; q < kSlotWords; q++) dst[q] = src[q];
    return;
  }
}

// cordahip_commit_log_revoke, two launches, one lane per row (commit_core.hpp's erase_row
// is the in-order statement). mark: the row's ref is looked up and the stored
// ConsumingTx compared; a match sets the slot's mark word (atomicOr: equal rows agree)
// and walks back to the first slot of its cluster, which it claims by compare-and-swap
// in a per-call scratch table keyed by that slot -- one matched row per cluster ends up
// with the start in owned[i], every other row with kNoCluster. No state word changes in
// this launch, so every lane measures the same clusters (the host keeps the load at or
// below 7/8, so every cluster has an empty slot before it and the walk ends there). repair: the owner of a cluster
// removes its marked entries (repair_cluster); clusters never share a slot that is
// written, so the owners are independent. counters[0] is the log's entry count,
// counters[1] the entries this call removed.
constexpr unsigned long long kNoCluster = ~0ull;

__global__ void __launch_bounds__(256) commit_revoke_mark_kernel(Table T, const uint32_t* __restrict__ rows,
                                                                 uint64_t n, unsigned long long* __restrict__ claim,
                                                                 uint64_t cmask, uint8_t* __restrict__ revoked,
                                                                 unsigned long long* __restrict__ owned,
                                                                 unsigned long long* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) counters[1] = 0;
  if (i >= n) return;
  const uint32_t* row = rows + i * (kRefWords + kByWords);
  const int64_t s = find(T, row, kNoFilter);
  const bool hit = s >= 0 && by_equal(T, (uint64_t)s, row + kRefWords);
  revoked[i] = hit;
  unsigned long long mine = kNoCluster;
  if (hit) {
    atomicOr(T.slots + (uint64_t)s * kSlotWords + kSlotMark, 1u);
    uint64_t start = (uint64_t)s;
    for (uint64_t k = 0; k <= T.mask && slot_state(T, (start - 1) & T.mask) != 0; k++) start = (start - 1) & T.mask;
    uint64_t c = (start * 0x9e3779b97f4a7c15ull >> 20) & cmask;
    for (uint64_t k = 0; k <= cmask; k++, c = (c + 1) & cmask) {
      const unsigned long long cur = atomicCAS(claim + c, kClaimEmpty, (unsigned long long)start);
      if (cur == kClaimEmpty) mine = start;
      if (cur == kClaimEmpty || cur == start) break;
    }
  }
  owned[i] = mine;
}

__global__ void __launch_bounds__(256) commit_revoke_repair_kernel(Table T, uint64_t n,
                                                                   const unsigned long long* __restrict__ owned,
                                                                   unsigned long long* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  long long removed = 0;
  if (i < n && owned[i] != kNoCluster) removed = (long long)repair_cluster(T, owned[i]);
  wave_add(counters, -removed);
  wave_add(counters + 1, removed);
}

// cordahip_commit_log_export, one lane per slot: a live slot whose sequence number
// (state - 1) is at least since_seq takes the next output index from *total -- one
// atomic per wave, the lanes ranked by their position among the wave's takers -- and
// writes its row and its sequence number when the index is below cap. *total ends as
// the number of matching entries.
__global__ void __launch_bounds__(256) commit_export_kernel(Table T, uint64_t since_seq, uint32_t* __restrict__ rows,
                                                            uint64_t* __restrict__ seq, uint64_t cap,
                                                            unsigned long long* __restrict__ total) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t st = i <= T.mask ? slot_state(T, i) : 0;
  const bool take = st != 0 && st - 1 >= since_seq;
  const unsigned long long takers = __ballot(take);
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long first = 0;
  if (lane == 0 && takers) first = atomicAdd(total, (unsigned long long)__popcll(takers));
  first = __shfl(first, 0, 64);
  const uint64_t at = first + (uint64_t)__popcll(takers & ((1ull << lane) - 1));
  if (!take || at >= cap) return;
  const uint32_t* w = T.slots + i * kSlotWords + kSlotRef;
  for (uint32_t q = 0; q < kRefWords + kByWords; q++) rows[at * (kRefWords + kByWords) + q] = w[q];
  seq[at] = st - 1;
}

// ---------------------------------------------------------------------------
// host-side launchers (called by cordahip.cpp)
static bool grid_of(uint64_t n, uint32_t* blocks) {
  const uint64_t b = (n + 255) / 256;
  *blocks = (uint32_t)b;
  return b <= 0x7fffffffull;
}

// CORDAHIP_COMMIT_ROUNDS: the parallel rounds before the in-order sweep (default 2)
static uint32_t commit_rounds() {
  static const uint32_t r = [] {
    const char* e = getenv("CORDAHIP_COMMIT_ROUNDS");
    const long v = e && *e ? strtol(e, nullptr, 10) : 2;
    return (uint32_t)(v < 0 ? 0 : v > 16 ? 16 : v);
  }();
  return r;
}

// the claim table of a call: a power of two of at least 2 n_refs slots
static uint64_t claim_slots(uint64_t n_refs) {
  uint64_t c = 64;
  while (c < 2 * n_refs) c *= 2;
  return c;
}

// scratch a commit call needs: the decisions, the clamped offsets, the undecided
// word, the claim table (with rounds on)
size_t commit_scratch_bytes(uint64_t ntx, uint64_t n_refs) {
  return (size_t)(((ntx + 15) & ~15ull) + (ntx + 2) * 8 + (commit_rounds() ? claim_slots(n_refs) * 8 : 0));
}

hipError_t launch_commit_inputs(const Table& T, Batch B, uint64_t n_refs, uint64_t base, void* scratch,
                                unsigned long long* entries, hipStream_t s) {
  if (B.ntx == 0) return hipSuccess;
  uint32_t g, g1;
  if (!grid_of(B.ntx, &g) || !grid_of(B.ntx + 1, &g1)) return hipErrorInvalidValue;
  uint8_t* decided = static_cast<uint8_t*>(scratch);
  uint64_t* off = reinterpret_cast<uint64_t*>(decided + ((B.ntx + 15) & ~15ull));
  unsigned long long* undecided = reinterpret_cast<unsigned long long*>(off + B.ntx + 1);
  unsigned long long* claim = undecided + 1;
  const uint64_t cslots = claim_slots(n_refs);
  hipLaunchKernelGGL(commit_clamp_kernel, dim3(g1), dim3(256), 0, s, B.off, B.ntx + 1, n_refs, off, undecided);
  B.off = off;
  hipLaunchKernelGGL(commit_prepass_kernel, dim3(g), dim3(256), 0, s, T, B, base, decided, undecided);
  for (uint32_t r = 0; r < commit_rounds(); r++) {
    if (const hipError_t e = hipMemsetAsync(claim, 0xff, cslots * 8, s)) return e;
    hipLaunchKernelGGL(commit_claim_kernel, dim3(g), dim3(256), 0, s, T, B, decided, claim, cslots - 1, undecided);
    hipLaunchKernelGGL(commit_win_kernel, dim3(g), dim3(256), 0, s, T, B, base, decided, claim, cslots - 1,
                       undecided, entries);
    hipLaunchKernelGGL(commit_lose_kernel, dim3(g), dim3(256), 0, s, T, B, base, decided, undecided);
  }
  hipLaunchKernelGGL(commit_sweep_kernel, dim3(1), dim3(64), 0, s, T, B, base, decided, undecided, entries);
  hipLaunchKernelGGL(commit_report_kernel, dim3(g), dim3(256), 0, s, T, B, base, decided);
  return hipGetLastError();
}

hipError_t launch_commit_lookup(const Table& T, const uint32_t* refs, uint64_t n, uint8_t* present, uint32_t* by,
                                hipStream_t s) {
  if (n == 0) return hipSuccess;
  uint32_t g;
  if (!grid_of(n, &g)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(commit_lookup_kernel, dim3(g), dim3(256), 0, s, T, refs, n, present, by);
  return hipGetLastError();
}

// scratch a load of n rows needs: a byte per row, then the claim table
size_t commit_load_scratch_bytes(uint64_t n) { return (size_t)(((n + 15) & ~15ull) + claim_slots(n) * 8); }

hipError_t launch_commit_load(const Table& T, const uint32_t* rows, uint64_t n, void* scratch,
                              unsigned long long* counters, hipStream_t s) {
  uint32_t g;
  if (n == 0 || !grid_of(n, &g)) return n ? hipErrorInvalidValue : hipSuccess;
  uint8_t* fresh = static_cast<uint8_t*>(scratch);
  unsigned long long* claim = reinterpret_cast<unsigned long long*>(fresh + ((n + 15) & ~15ull));
  const uint64_t cslots = claim_slots(n);
  if (const hipError_t e = hipMemsetAsync(claim, 0xff, cslots * 8, s)) return e;
  hipLaunchKernelGGL(commit_load_claim_kernel, dim3(g), dim3(256), 0, s, T, rows, n, claim, cslots - 1, fresh, counters);
  hipLaunchKernelGGL(commit_load_insert_kernel, dim3(g), dim3(256), 0, s, T, rows, n, claim, cslots - 1, fresh,
                     counters);
  return hipGetLastError();
}

// scratch a revoke of n rows needs: a cluster start per row, then the claim table
size_t commit_revoke_scratch_bytes(uint64_t n) { return (size_t)(n * 8 + claim_slots(n) * 8); }

hipError_t launch_commit_revoke(const Table& T, const uint32_t* rows, uint64_t n, uint8_t* revoked, void* scratch,
                                unsigned long long* counters, hipStream_t s) {
  uint32_t g;
  if (n == 0 || !grid_of(n, &g)) return n ? hipErrorInvalidValue : hipSuccess;
  unsigned long long* owned = static_cast<unsigned long long*>(scratch);
  unsigned long long* claim = owned + n;
  const uint64_t cslots = claim_slots(n);
  if (const hipError_t e = hipMemsetAsync(claim, 0xff, cslots * 8, s)) return e;
  hipLaunchKernelGGL(commit_revoke_mark_kernel, dim3(g), dim3(256), 0, s, T, rows, n, claim, cslots - 1, revoked, owned,
                     counters);
  hipLaunchKernelGGL(commit_revoke_repair_kernel, dim3(g), dim3(256), 0, s, T, n, owned, counters);
  return hipGetLastError();
}

hipError_t launch_commit_export(const Table& T, uint64_t since_seq, uint32_t* rows, uint64_t* seq, uint64_t cap,
                                unsigned long long* total, hipStream_t s) {
  uint32_t g;
  if (!grid_of(T.mask + 1, &g)) return hipErrorInvalidValue;
  if (const hipError_t e = hipMemsetAsync(total, 0, 8, s)) return e;
  hipLaunchKernelGGL(commit_export_kernel, dim3(g), dim3(256), 0, s, T, since_seq, rows, seq, cap, total);
  return hipGetLastError();
}

hipError_t launch_commit_rehash(const Table& from, const Table& to, hipStream_t s) {
  uint32_t g;
  if (!grid_of(from.mask + 1, &g)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(commit_rehash_kernel, dim3(g), dim3(256), 0, s, from, to);
  return hipGetLastError();
}

}  // namespace cordahip
