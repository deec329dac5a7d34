// Mutation fuzzing of cordahip_commit_inputs' validation on the host, built with
// ASan + UBSan by tests/test_commit_csr_fuzz.py (no HIP, no device): commit batches
// whose every array sits in a heap block of exactly its declared entries; tx_ref_off
// entries, n_refs, ntx, now_ns, tolerance_ns and the pairing of the window arrays
// are mutated; check_commit (csr_check.hpp) must accept exactly the batches an
// independent statement of the contract accepts (offsets non-decreasing, the last
// within n_refs, |now| < 2^61, 0 <= tolerance < 2^61, both window arrays or none).
// A batch it accepts then runs through the host instance of the commit core
// (commit_core.hpp run_serial) over those exact-size blocks and an exact-size
// table, so a read outside a caller array or a write outside an output is a
// sanitizer report; window sides sit at and beyond the saturation bounds +-2^62
// and now / tolerance at the edge of their range, where a difference that
// overflowed would be a UBSan report.
// Usage: commit_csr_fuzz <batches> <seed>; prints one JSON line, exit 0 = pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../corda_amd/csrc/commit_core.hpp"
#include "../corda_amd/csrc/csr_check.hpp"

using namespace cordahip::rt;
using namespace cordahip::commit;

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return n ? next() % n : 0; }
  bool chance(uint64_t pct) { return below(100) < pct; }
};

// an exact-size heap array (an empty one still has a distinct, unreadable address)
template <class T>
struct Arr {
  std::unique_ptr<T[]> p;
  void from(const std::vector<T>& v) {
    p.reset(new T[v.size()]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), sizeof(T) * v.size());
  }
  void make(uint64_t k, int fill) {
    p.reset(new T[k]);
    if (k) std::memset(p.get(), fill, sizeof(T) * k);
  }
  T* get() const { return p.get(); }
};

struct SerialPar {
  template <class F>
  void operator()(uint64_t n, uint64_t, F&& fn) const {
    if (n) fn(0, n);
  }
};

// the contract, restated
bool contract_ok(const std::vector<uint64_t>& off, uint64_t ntx, uint64_t n_refs, int64_t now, int64_t tol, bool from,
                 bool until) {
  const int64_t lim = 2305843009213693952ll;  // 2^61
  if (!(now > -lim && now < lim) || !(tol >= 0 && tol < lim)) return false;
  if (from != until) return false;
  for (uint64_t t = 0; t < ntx; t++)
    if (off[t] > off[t + 1]) return false;
  return ntx == 0 || off[ntx] <= n_refs;
}

struct Stats {
  uint64_t batches = 0, invalid = 0, ran = 0, txs = 0, refs = 0, committed = 0, window_invalid = 0, edge_scalars = 0;
};

bool one(Rng& rng, Stats& st) {
  uint64_t ntx = rng.below(40);
  std::vector<uint64_t> off(ntx + 1, 0);
  off[0] = rng.chance(20) ? rng.below(4) : 0;  // a batch may start inside refs
  for (uint64_t t = 0; t < ntx; t++) off[t + 1] = off[t] + rng.below(6);
  uint64_t n_refs = off[ntx] + (rng.chance(30) ? rng.below(5) : 0);
  const int64_t lim = (int64_t)1 << 61;
  int64_t now = (int64_t)rng.below(2000001) - 1000000, tol = (int64_t)rng.below(5000);
  bool has_from = rng.chance(70), has_until = has_from;
  if (rng.chance(15)) {  // the ends of the scalars' ranges: valid
    now = rng.chance(50) ? lim - 1 : -(lim - 1);
    tol = rng.chance(50) ? lim - 1 : 0;
    st.edge_scalars++;
  }
  // mutations
  if (rng.chance(45)) {
    switch (rng.below(8)) {
      case 0:
        if (ntx) off[rng.below(ntx + 1)] = rng.chance(50) ? rng.next() : rng.below(n_refs + 3);
        break;
      case 1:
        n_refs = rng.chance(50) ? rng.below(off[ntx] + 1) : off[ntx] ? off[ntx] - 1 : 0;
        break;
      case 2: {  // more or fewer transactions than the offsets were built for
        const uint64_t k = rng.below(45);
        off.resize(k + 1, rng.chance(50) ? off.back() : rng.below(n_refs + 2));
        ntx = k;
        break;
      }
      case 3:
        now = rng.chance(50) ? lim : rng.chance(50) ? -lim : (int64_t)rng.next();
        break;
      case 4:
        tol = rng.chance(50) ? lim : rng.chance(50) ? -1 : (int64_t)rng.next();
        break;
      case 5:
        has_from = !has_until;
        break;
      case 6:
        if (ntx > 1) std::swap(off[rng.below(ntx + 1)], off[rng.below(ntx + 1)]);
        break;
      default:
        if (ntx) off[ntx] = n_refs + 1 + rng.below(3);
        break;
    }
  }
  // every array in a block of exactly its declared entries
  Arr<uint64_t> a_off;
  a_off.from(off);
  std::vector<int64_t> from(ntx), until(ntx);
  const int64_t sat = (int64_t)1 << 62;
  const int64_t n0 = now > -lim && now < lim ? now : 0, t0 = tol >= 0 && tol < lim ? tol : 0;  // rejected anyway
  for (uint64_t t = 0; t < ntx; t++) {
    // absent, at the saturation bounds, beyond them (a caller that did not saturate), near now
    const int64_t side[8] = {kSideAbsent, sat,     -sat,    n0 + t0, n0 - t0, n0 / 2 + (int64_t)rng.below(100) - 50,
                             INT64_MAX,   INT64_MIN + 1};
    from[t] = side[rng.below(8)];
    until[t] = side[rng.below(8)];
  }
  Arr<int64_t> a_from, a_until;
  a_from.from(from);
  a_until.from(until);
  Arr<uint32_t> a_txid, a_caller, a_refs, a_by;
  Arr<uint8_t> a_gate, a_status, a_comm, a_state;
  std::vector<uint32_t> txid(ntx * 8), caller(ntx), refs(n_refs * kRefWords);
  for (auto& w : txid) w = (uint32_t)rng.below(4);
  for (auto& w : caller) w = (uint32_t)rng.below(3);
  for (uint64_t i = 0; i < n_refs; i++) refs[i * kRefWords] = (uint32_t)rng.below(24);  // a small universe: collisions
  std::vector<uint8_t> gate(ntx);
  for (auto& g : gate) g = rng.chance(10);
  a_txid.from(txid);
  a_caller.from(caller);
  a_refs.from(refs);
  a_gate.from(gate);
  a_status.make(ntx, 0xee);
  a_comm.make(ntx, 0xee);
  a_state.make(n_refs, 0xee);
  a_by.make(n_refs * kByWords, 0xee);

  cordahip_commit_batch b{};
  b.ntx = ntx;
  b.txid = reinterpret_cast<const uint8_t*>(a_txid.get());
  b.caller = a_caller.get();
  b.refs = reinterpret_cast<const cordahip_state_ref*>(a_refs.get());
  b.tx_ref_off = a_off.get();
  b.n_refs = n_refs;
  b.tw_from = has_from ? a_from.get() : nullptr;
  b.tw_until = has_until ? a_until.get() : nullptr;
  b.now_ns = now;
  b.tolerance_ns = tol;
  b.gate = rng.chance(50) ? a_gate.get() : nullptr;
  b.tx_status = a_status.get();
  b.committed = a_comm.get();
  b.ref_state = a_state.get();
  b.ref_by = reinterpret_cast<cordahip_consuming_tx*>(a_by.get());

  st.batches++;
  const bool want = contract_ok(off, ntx, n_refs, now, tol, has_from, has_until);
  const bool got = check_commit(SerialPar{}, &b);
  if (want != got) {
    fprintf(stderr, "verdicts differ: contract %d, check_commit %d (ntx %llu, n_refs %llu)\n", (int)want, (int)got,
            (unsigned long long)ntx, (unsigned long long)n_refs);
    return false;
  }
  if (!got) {
    st.invalid++;
    return true;
  }
  // an accepted batch through the host core: a table that keeps n_refs entries below 7/8 load
  uint64_t cap = 64;
  while (cap / 8 * 7 < n_refs) cap *= 2;
  Arr<uint32_t> slots;
  slots.make(cap * kSlotWords, 0);
  const Table T{slots.get(), cap - 1, rng.next(), rng.next()};
  Batch B{};
  B.ntx = ntx;
  B.txid = a_txid.get();
  B.caller = a_caller.get();
  B.refs = a_refs.get();
  B.off = a_off.get();
  B.tw_from = b.tw_from;
  B.tw_until = b.tw_until;
  B.now_ns = now;
  B.tolerance_ns = tol;
  B.gate = b.gate;
  B.tx_status = a_status.get();
  B.committed = a_comm.get();
  B.ref_state = a_state.get();
  B.ref_by = a_by.get();
  const uint64_t added = run_serial(T, B, 1);
  st.ran++;
  st.txs += ntx;
  uint64_t span = ntx ? off[ntx] - off[0] : 0;
  st.refs += span;
  if (added > span) return false;
  for (uint64_t t = 0; t < ntx; t++) {
    const uint8_t s = a_status.get()[t], c = a_comm.get()[t];
    if (s != kCommitOk && s != kCommitConflict && s != kCommitTimeWindowInvalid && s != kCommitSkipped) return false;
    if (c > 1 || (c && s != kCommitOk)) return false;
    st.committed += c;
    st.window_invalid += s == kCommitTimeWindowInvalid;
  }
  // rows outside [off[0], off[ntx]) stay untouched
  for (uint64_t i = 0; i < n_refs; i++)
    if ((ntx == 0 || i < off[0] || i >= off[ntx]) && a_state.get()[i] != 0xee) return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t batches = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
  Rng rng{argc > 2 ? strtoull(argv[2], nullptr, 10) : 1};
  Stats st;
  bool ok = true;
  for (uint64_t i = 0; i < batches && ok; i++) ok = one(rng, st);
  printf("{\"ok\": %s, \"batches\": %llu, \"invalid\": %llu, \"ran\": %llu, \"txs\": %llu, \"refs\": %llu, "
         "\"committed\": %llu, \"window_invalid\": %llu, \"edge_scalars\": %llu}\n",
         ok ? "true" : "false", (unsigned long long)st.batches, (unsigned long long)st.invalid,
         (unsigned long long)st.ran, (unsigned long long)st.txs, (unsigned long long)st.refs,
         (unsigned long long)st.committed, (unsigned long long)st.window_invalid, (unsigned long long)st.edge_scalars);
  return ok ? 0 : 1;
}
