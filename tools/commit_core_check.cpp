// The commit log's core (corda_amd/csrc/commit_core.hpp: keyed slot index, probing,
// the time-window rule, the in-order commit and the report) on the host against an
// independent std::map model, built with ASan + UBSan by tests/test_commit_core_check.py
// (no HIP, no device). Seeded batches over a dense universe: refs from 40 values, 8
// transaction ids, 3 callers, 0-5 inputs per transaction, gates and time windows; the
// table is 64 slots in a heap block of exactly its size, pre-loaded so that it runs at up
// to 7/8 load (56 entries) and probe sequences wrap its end. After every batch every
// status, committed byte, ref_state and ref_by row is compared with the model's, and
// every ref of the universe is looked up and compared with the map.
// Usage: commit_core_check <rounds> <seed>; prints one JSON line, exit 0 = pass.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "../corda_amd/csrc/commit_core.hpp"

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

using Ref = std::array<uint32_t, kRefWords>;
using By = std::array<uint32_t, kByWords>;

Ref make_ref(uint64_t salt, uint32_t v) {
  Ref r;
  Rng g{salt * 1000003ull + v};
  for (uint32_t i = 0; i < 8; i++) r[i] = (uint32_t)g.next();
  r[8] = v % 3;  // several refs share an output index
  return r;
}

struct Stats {
  uint64_t batches = 0, txs = 0, committed = 0, already = 0, conflicts = 0, skipped = 0, window_invalid = 0,
           max_entries = 0, wrapped = 0, lookups = 0, loads_dup = 0, failures = 0;
};

// the entry's slot lies before the slot its hash names: the probe wrapped the table's end
bool wrapped(const Table& T, const uint32_t* ref, int64_t slot) {
  return slot >= 0 && (uint64_t)slot < (hash_ref(ref, T.k0, T.k1) & T.mask);
}

bool run_round(Rng& rng, Stats& st) {
  const uint64_t cap = 64;
  std::unique_ptr<uint32_t[]> slots(new uint32_t[cap * kSlotWords]);  // exact size: a probe past the end is a report
  std::memset(slots.get(), 0, cap * kSlotWords * 4);
  const Table T{slots.get(), cap - 1, rng.next(), rng.next()};
  const uint64_t world = rng.next();
  std::map<Ref, By> model;
  uint64_t base = 1;

  // start-up load: up to 16 refs outside the universe (so 40 universe refs reach 56), some twice
  const uint64_t nload = rng.chance(40) ? 16 : rng.below(17);
  uint64_t dup = 0, dup_model = 0;
  for (uint64_t i = 0; i < nload + 3; i++) {
    const uint32_t v = 1000 + (uint32_t)(i < nload ? i : rng.below(nload ? nload : 1));
    if (i >= nload && nload == 0) break;
    uint32_t row[kRefWords + kByWords];
    const Ref r = make_ref(world, v);
    std::memcpy(row, r.data(), sizeof(r));
    for (uint32_t q = 0; q < kByWords; q++) row[kRefWords + q] = (uint32_t)rng.next();
    const int got = load_row(T, row);
    By by;
    std::memcpy(by.data(), row + kRefWords, sizeof(by));
    const bool fresh = model.emplace(r, by).second;
    if ((got == 1) != fresh) return false;
    dup += got == 0;
    dup_model += !fresh;
  }
  if (dup != dup_model) return false;
  st.loads_dup += dup;

  const uint64_t nbatches = 1 + rng.below(10);
  for (uint64_t bi = 0; bi < nbatches; bi++) {
    const uint64_t ntx = rng.below(24);
    std::vector<uint32_t> txid(ntx * 8 + 1), caller(ntx + 1);
    std::vector<uint64_t> off(ntx + 1, 0);
    std::vector<Ref> refs;
    std::vector<int64_t> from(ntx + 1), until(ntx + 1);
    std::vector<uint8_t> gate(ntx + 1);
    const bool windows = rng.chance(60), gated = rng.chance(50);
    const int64_t now = (int64_t)rng.below(1000000) - 500000, tol = (int64_t)rng.below(1000);
    for (uint64_t t = 0; t < ntx; t++) {
      const uint32_t id = (uint32_t)rng.below(8);
      Rng g{world ^ (0xabcdull + id)};
      for (uint32_t q = 0; q < 8; q++) txid[t * 8 + q] = (uint32_t)g.next();
      caller[t] = (uint32_t)rng.below(3);
      const uint64_t k = rng.below(6);
      for (uint64_t i = 0; i < k; i++) refs.push_back(make_ref(world, (uint32_t)rng.below(40)));
      off[t + 1] = refs.size();
      // windows around now: exactly at the tolerance, one ns past it, absent sides
      const int64_t edge[4] = {tol, tol + 1, 0, -5};
      from[t] = rng.chance(30) ? kSideAbsent : now + edge[rng.below(4)];
      until[t] = rng.chance(30) ? kSideAbsent : now - edge[rng.below(4)];
      gate[t] = rng.chance(15) ? (uint8_t)(1 + rng.below(255)) : 0;
    }
    const uint64_t nr = refs.size();
    // exact-size blocks for what the core indexes by input
    std::unique_ptr<uint32_t[]> rw(new uint32_t[nr * kRefWords + 1]), by(new uint32_t[nr * kByWords + 1]);
    std::unique_ptr<uint8_t[]> rstate(new uint8_t[nr + 1]), status(new uint8_t[ntx + 1]), comm(new uint8_t[ntx + 1]);
    for (uint64_t i = 0; i < nr; i++) std::memcpy(rw.get() + i * kRefWords, refs[i].data(), sizeof(Ref));
    std::memset(by.get(), 0xee, (nr * kByWords + 1) * 4);
    std::memset(rstate.get(), 0xee, nr + 1);
    std::memset(status.get(), 0xee, ntx + 1);
    std::memset(comm.get(), 0xee, ntx + 1);
    Batch B{};
    B.ntx = ntx;
    B.txid = txid.data();
    B.caller = caller.data();
    B.refs = rw.get();
    B.off = off.data();
    B.tw_from = windows ? from.data() : nullptr;
    B.tw_until = windows ? until.data() : nullptr;
    B.now_ns = now;
    B.tolerance_ns = tol;
    B.gate = gated ? gate.data() : nullptr;
    B.tx_status = status.get();
    B.committed = comm.get();
    B.ref_state = rstate.get();
    B.ref_by = by.get();
    const uint64_t before = model.size();
    const uint64_t added = run_serial(T, B, base);

    // the model, from the statement of the provider: a map, one transaction at a time
    for (uint64_t t = 0; t < ntx; t++) {
      st.txs++;
      uint8_t want = kCommitOk, want_comm = 0;
      std::vector<uint8_t> ws(off[t + 1] - off[t], kRefAbsent);
      std::vector<By> wb(ws.size(), By{});
      By mine;
      for (uint32_t q = 0; q < 8; q++) mine[q] = txid[t * 8 + q];
      mine[9] = caller[t];
      bool invalid = false;
      if (windows) {
        // restated with 128-bit differences
        const __int128 n128 = now, t128 = tol;
        if (until[t] != kSideAbsent && n128 - (__int128)until[t] > t128) invalid = true;
        if (from[t] != kSideAbsent && (__int128)from[t] - n128 > t128) invalid = true;
      }
      if (gated && gate[t]) {
        want = kCommitSkipped;
        st.skipped++;
      } else if (invalid) {
        want = kCommitTimeWindowInvalid;
        st.window_invalid++;
      } else {
        bool any = false, other = false;
        for (uint64_t i = off[t]; i < off[t + 1]; i++) {
          const auto it = model.find(refs[i]);
          if (it == model.end()) continue;
          any = true;
          mine[8] = (uint32_t)(i - off[t]);
          wb[i - off[t]] = it->second;
          ws[i - off[t]] = it->second == mine ? kRefSelf : kRefOther;
          other |= !(it->second == mine);
        }
        if (!any) {
          for (uint64_t i = off[t]; i < off[t + 1]; i++) {
            mine[8] = (uint32_t)(i - off[t]);
            model[refs[i]] = mine;
          }
          want_comm = 1;
          st.committed++;
        } else if (other) {
          want = kCommitConflict;
          st.conflicts++;
        } else {
          st.already++;
        }
      }
      if (status[t] != want || comm[t] != want_comm) return false;
      for (uint64_t i = off[t]; i < off[t + 1]; i++) {
        if (rstate[i] != ws[i - off[t]]) return false;
        if (std::memcmp(by.get() + i * kByWords, wb[i - off[t]].data(), sizeof(By)) != 0) return false;
      }
    }
    if (added != model.size() - before) return false;
    if (status[ntx] != 0xee || comm[ntx] != 0xee || rstate[nr] != 0xee || by[nr * kByWords] != 0xeeeeeeeeu) return false;
    base += ntx;
    st.batches++;
    if (model.size() > st.max_entries) st.max_entries = model.size();
    if (model.size() > 56) return false;  // the generator keeps the table at or below 7/8

    // the whole universe (and the loaded fillers) against the map
    for (uint32_t v = 0; v < 40 + 16; v++) {
      const Ref r = make_ref(world, v < 40 ? v : 1000 + (v - 40));
      const int64_t s = find(T, r.data(), kNoFilter);
      const auto it = model.find(r);
      st.lookups++;
      if ((s >= 0) != (it != model.end())) return false;
      if (s < 0) continue;
      st.wrapped += wrapped(T, r.data(), s);
      if (std::memcmp(T.slots + (uint64_t)s * kSlotWords + kSlotBy, it->second.data(), sizeof(By)) != 0) return false;
    }
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t rounds = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000;
  Rng rng{argc > 2 ? strtoull(argv[2], nullptr, 10) : 1};
  Stats st;
  for (uint64_t r = 0; r < rounds; r++)
    if (!run_round(rng, st)) {
      st.failures++;
      fprintf(stderr, "round %llu failed\n", (unsigned long long)r);
      break;
    }
  printf("{\"ok\": %s, \"failures\": %llu, \"rounds\": %llu, \"batches\": %llu, \"txs\": %llu, \"committed\": %llu, "
         "\"already\": %llu, \"conflicts\": %llu, \"skipped\": %llu, \"window_invalid\": %llu, \"max_entries\": %llu, "
         "\"wrapped\": %llu, \"lookups\": %llu, \"loads_dup\": %llu}\n",
         st.failures ? "false" : "true", (unsigned long long)st.failures, (unsigned long long)rounds,
         (unsigned long long)st.batches, (unsigned long long)st.txs, (unsigned long long)st.committed,
         (unsigned long long)st.already, (unsigned long long)st.conflicts, (unsigned long long)st.skipped,
         (unsigned long long)st.window_invalid, (unsigned long long)st.max_entries, (unsigned long long)st.wrapped,
         (unsigned long long)st.lookups, (unsigned long long)st.loads_dup);
  return st.failures ? 1 : 0;
}
