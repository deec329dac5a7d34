// The commit log's removal (corda_amd/csrc/commit_core.hpp: erase_at, erase_row,
// repair_cluster -- the code cordahip_commit_log_revoke's kernels run) on the host
// against an independent std::map model, built with ASan + UBSan by
// tests/test_commit_erase_check.py (no HIP, no device). The table is 64 slots in a heap
// block of exactly its size, at up to 7/8 load (56 entries: 40 universe refs and 16
// fillers); seeded interleavings of load_row, run_serial batches (8 transaction ids, 3
// callers, 0-4 inputs), erase_row calls (matching rows, rows with another id, position or
// caller, absent refs) and whole revokes: a subset of rows is applied row by row with
// erase_row to one copy of the table, and marked and repaired cluster by cluster, the
// clusters in shuffled order, in another; the two are compared slot for slot in
// occupancy. After every step every ref of the universe is looked up and compared with
// the map, and the table's structure is checked: no empty slot between any entry's home
// and its slot (cyclically), every empty slot zero in all its words, no mark left.
// Usage: commit_erase_check <rounds> <seed>; prints one JSON line, exit 0 = pass.
//        commit_erase_check --hash: hash_ref of a few fixed refs and keys, one JSON line.
#include <algorithm>
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
using Row = std::array<uint32_t, kRefWords + kByWords>;
constexpr uint64_t kCap = 64, kUniverse = 40, kFillers = 16, kMaxEntries = 56;

Ref make_ref(uint64_t salt, uint32_t v) {
  Ref r;
  Rng g{salt * 1000003ull + v};
  for (uint32_t i = 0; i < 8; i++) r[i] = (uint32_t)g.next();
  r[8] = v % 3;
  return r;
}
Ref universe_ref(uint64_t world, uint32_t v) { return make_ref(world, v < kUniverse ? v : 1000 + (v - (uint32_t)kUniverse)); }

struct Stats {
  uint64_t steps = 0, loads = 0, batches = 0, committed = 0, removals = 0, refused_absent = 0, refused_id = 0,
           refused_index = 0, refused_caller = 0, wrap_shifts = 0, erased_cluster_starts = 0, cluster_splits = 0,
           revokes = 0, revoke_rows = 0, revoke_removed = 0, adjacent_marked = 0, wrapping_clusters_repaired = 0,
           max_entries = 0, lookups = 0, failures = 0;
};

struct Owned {
  std::unique_ptr<uint32_t[]> words;  // exact size: a probe or a shift past the end is a report
  Table T;
  Owned(uint64_t k0, uint64_t k1) : words(new uint32_t[kCap * kSlotWords]), T{words.get(), kCap - 1, k0, k1} {
    std::memset(words.get(), 0, kCap * kSlotWords * 4);
  }
  Owned(const Owned& o) : words(new uint32_t[kCap * kSlotWords]), T{words.get(), kCap - 1, o.T.k0, o.T.k1} {
    std::memcpy(words.get(), o.words.get(), kCap * kSlotWords * 4);
  }
};

bool occupied(const Table& T, uint64_t s) { return slot_state(T, s & T.mask) != 0; }

// no empty slot between an entry's home and its slot; empty slots zero; no mark anywhere
bool structure_ok(const Table& T) {
  for (uint64_t s = 0; s <= T.mask; s++) {
    const uint32_t* w = T.slots + s * kSlotWords;
    if (!occupied(T, s)) {
      for (uint32_t q = 0; q < kSlotWords; q++)
        if (w[q]) return false;
      continue;
    }
    if (w[kSlotMark] || w[kSlotMark + 1] || w[kSlotMark + 2]) return false;
    for (uint64_t h = hash_ref(w + kSlotRef, T.k0, T.k1) & T.mask; h != s; h = (h + 1) & T.mask)
      if (!occupied(T, h)) return false;
  }
  return true;
}

bool universe_ok(const Table& T, uint64_t world, const std::map<Ref, By>& model, Stats& st) {
  uint64_t live = 0;
  for (uint64_t s = 0; s <= T.mask; s++) live += occupied(T, s);
  if (live != model.size()) return false;
  for (uint32_t v = 0; v < kUniverse + kFillers; v++) {
    const Ref r = universe_ref(world, v);
    const int64_t s = find(T, r.data(), kNoFilter);
    const auto it = model.find(r);
    st.lookups++;
    if ((s >= 0) != (it != model.end())) return false;
    if (s >= 0 && std::memcmp(T.slots + (uint64_t)s * kSlotWords + kSlotBy, it->second.data(), sizeof(By)) != 0)
      return false;
  }
  return true;
}

By tx_by(uint64_t world, uint32_t id, uint32_t index, uint32_t caller) {
  By b;
  Rng g{world ^ (0xabcdull + id)};
  for (uint32_t q = 0; q < 8; q++) b[q] = (uint32_t)g.next();
  b[8] = index;
  b[9] = caller;
  return b;
}

// A row for erase_row about universe ref v, and what the model says of it: 1 removes.
// kind: 0 matching / absent, 1 another id, 2 another position, 3 another caller.
Row make_row(Rng& rng, uint64_t world, const std::map<Ref, By>& model, uint32_t v, int* kind, bool* live) {
  const Ref r = universe_ref(world, v);
  const auto it = model.find(r);
  *live = it != model.end();
  By by = *live ? it->second : tx_by(world, (uint32_t)rng.below(8), 0, 0);
  *kind = *live && rng.chance(45) ? 1 + (int)rng.below(3) : 0;
  if (*kind == 1) by[rng.below(8)] ^= 1u << rng.below(32);
  if (*kind == 2) by[8] += 1 + (uint32_t)rng.below(3);
  if (*kind == 3) by[9] ^= 1u << rng.below(32);
  Row row;
  std::memcpy(row.data(), r.data(), sizeof(Ref));
  std::memcpy(row.data() + kRefWords, by.data(), sizeof(By));
  return row;
}

// erase_row on T with the model, and what the removal did to the table's shape
bool erase_step(const Table& T, const Row& row, int kind, bool live, std::map<Ref, By>& model, Stats& st) {
  Ref r;
  std::memcpy(r.data(), row.data(), sizeof(Ref));
  const bool want = live && kind == 0;
  uint8_t occ[kCap];
  for (uint64_t s = 0; s < kCap; s++) occ[s] = occupied(T, s);
  const int64_t at = find(T, r.data(), kNoFilter);
  std::vector<Ref> keys(kCap);
  for (uint64_t s = 0; s < kCap; s++)
    if (occ[s]) std::memcpy(keys[s].data(), T.slots + s * kSlotWords + kSlotRef, sizeof(Ref));
  const int got = erase_row(T, row.data());
  if (got != (want ? 1 : 0)) return false;
  if (!want) {
    (!live ? st.refused_absent : kind == 1 ? st.refused_id : kind == 2 ? st.refused_index : st.refused_caller)++;
    for (uint64_t s = 0; s < kCap; s++)
      if (occ[s] != occupied(T, s)) return false;
    return true;
  }
  model.erase(r);
  st.removals++;
  st.erased_cluster_starts += !occ[(at - 1) & (kCap - 1)];
  uint64_t cleared = 0, ncleared = 0;
  for (uint64_t s = 0; s < kCap; s++) {
    if (occ[s] && !occupied(T, s)) cleared = s, ncleared++;
    if (!occ[s] && occupied(T, s)) return false;  // a shift never fills a slot that was empty
    if (!occ[s] || (int64_t)s == at) continue;
    const int64_t now = find(T, keys[s].data(), kNoFilter);
    if (now < 0) return false;
    st.wrap_shifts += (uint64_t)now > s;  // moved back across the table's end
  }
  if (ncleared != 1) return false;
  st.cluster_splits += occupied(T, cleared + kCap - 1) && occupied(T, cleared + 1);
  return true;
}

// One whole revoke two ways: erase_row row by row on A; mark + per-cluster repair on B.
bool revoke_step(Rng& rng, Owned& A, uint64_t world, std::map<Ref, By>& model, Stats& st) {
  Owned B(A);
  const uint64_t n = rng.below(24);
  uint64_t removed_a = 0, marked = 0;
  Row row{};
  for (uint64_t i = 0; i < n; i++) {
    int kind;
    bool live;
    if (i == 0 || !rng.chance(15))  // else the previous row once more
      row = make_row(rng, world, model, (uint32_t)rng.below(kUniverse + kFillers), &kind, &live);
    // the mark launch: every row against the table as it stood before the call
    const int64_t s = find(B.T, row.data(), kNoFilter);
    const bool hit = s >= 0 && by_equal(B.T, (uint64_t)s, row.data() + kRefWords);
    if (hit) {
      marked += B.T.slots[(uint64_t)s * kSlotWords + kSlotMark] == 0;
      B.T.slots[(uint64_t)s * kSlotWords + kSlotMark] |= 1u;
    }
    // in order: a repeated row finds its entry gone, which is the same entry counted once
    Ref r;
    std::memcpy(r.data(), row.data(), sizeof(Ref));
    const int got = erase_row(A.T, row.data());
    if (got) model.erase(r);
    if (got && !hit) return false;
    removed_a += got;
    st.revoke_rows++;
  }
  if (removed_a != marked) return false;
  std::vector<uint64_t> starts;
  for (uint64_t s = 0; s < kCap; s++) {
    if (!occupied(B.T, s)) continue;
    const bool m = B.T.slots[s * kSlotWords + kSlotMark] != 0;
    st.adjacent_marked += m && occupied(B.T, s + 1) && B.T.slots[((s + 1) & (kCap - 1)) * kSlotWords + kSlotMark] != 0;
    if (!occupied(B.T, s + kCap - 1)) starts.push_back(s);
  }
  for (uint64_t i = starts.size(); i > 1; i--) std::swap(starts[i - 1], starts[rng.below(i)]);
  uint64_t removed_b = 0;
  for (const uint64_t c : starts) {
    uint64_t len = 0;
    while (occupied(B.T, c + len)) len++;
    const uint64_t r = repair_cluster(B.T, c);
    st.wrapping_clusters_repaired += r > 0 && c + len > kCap;
    removed_b += r;
  }
  if (removed_b != removed_a) return false;
  for (uint64_t s = 0; s < kCap; s++)
    if (occupied(A.T, s) != occupied(B.T, s)) return false;
  if (!structure_ok(B.T) || !universe_ok(B.T, world, model, st)) return false;
  st.revokes++;
  st.revoke_removed += removed_a;
  return true;
}

bool batch_step(Rng& rng, const Table& T, uint64_t world, std::map<Ref, By>& model, uint64_t* base, Stats& st) {
  const uint64_t ntx = 1 + rng.below(10);
  std::vector<uint32_t> txid(ntx * 8), caller(ntx), ids(ntx);
  std::vector<uint64_t> off(ntx + 1, 0);
  std::vector<Ref> refs;
  uint64_t room = kMaxEntries - model.size();
  for (uint64_t t = 0; t < ntx; t++) {
    ids[t] = (uint32_t)rng.below(8);
    const By b = tx_by(world, ids[t], 0, 0);
    std::memcpy(txid.data() + t * 8, b.data(), 32);
    caller[t] = (uint32_t)rng.below(3);
    uint64_t k = rng.below(5);
    k = k < room ? k : room;  // the generator keeps the table at or below 7/8
    room -= k;
    for (uint64_t i = 0; i < k; i++) refs.push_back(make_ref(world, (uint32_t)rng.below(kUniverse)));
    off[t + 1] = refs.size();
  }
  const uint64_t nr = refs.size();
  std::unique_ptr<uint32_t[]> rw(new uint32_t[nr * kRefWords + 1]), by(new uint32_t[nr * kByWords + 1]);
  std::unique_ptr<uint8_t[]> rstate(new uint8_t[nr + 1]), status(new uint8_t[ntx]), comm(new uint8_t[ntx]);
  for (uint64_t i = 0; i < nr; i++) std::memcpy(rw.get() + i * kRefWords, refs[i].data(), sizeof(Ref));
  Batch B{};
  B.ntx = ntx;
  B.txid = txid.data();
  B.caller = caller.data();
  B.refs = rw.get();
  B.off = off.data();
  B.tx_status = status.get();
  B.committed = comm.get();
  B.ref_state = rstate.get();
  B.ref_by = by.get();
  (void)run_serial(T, B, *base);
  *base += ntx;
  for (uint64_t t = 0; t < ntx; t++) {
    bool any = false;
    for (uint64_t i = off[t]; i < off[t + 1]; i++) any |= model.count(refs[i]) != 0;
    if (comm[t] != (any ? 0 : 1)) return false;
    if (any) continue;
    for (uint64_t i = off[t]; i < off[t + 1]; i++) model[refs[i]] = tx_by(world, ids[t], (uint32_t)(i - off[t]), caller[t]);
    st.committed++;
  }
  st.batches++;
  return true;
}

bool run_round(Rng& rng, Stats& st) {
  Owned A(rng.next(), rng.next());
  const Table& T = A.T;
  const uint64_t world = rng.next();
  std::map<Ref, By> model;
  uint64_t base = 1;
  const uint64_t nsteps = 8 + rng.below(40);
  for (uint64_t k = 0; k < nsteps; k++) {
    const uint64_t what = rng.below(100);
    if (what < 25) {  // a load of fillers and universe refs, some present already
      const uint64_t n = rng.below(12);
      for (uint64_t i = 0; i < n && model.size() < kMaxEntries; i++) {
        const Ref r = universe_ref(world, (uint32_t)rng.below(kUniverse + kFillers));
        Row row;
        std::memcpy(row.data(), r.data(), sizeof(Ref));
        for (uint32_t q = 0; q < kByWords; q++) row[kRefWords + q] = (uint32_t)rng.next();
        By b;
        std::memcpy(b.data(), row.data() + kRefWords, sizeof(By));
        if ((load_row(T, row.data()) == 1) != model.emplace(r, b).second) return false;
      }
      st.loads++;
    } else if (what < 50) {
      if (!batch_step(rng, T, world, model, &base, st)) return false;
    } else if (what < 85) {
      int kind;
      bool live;
      const Row row = make_row(rng, world, model, (uint32_t)rng.below(kUniverse + kFillers), &kind, &live);
      if (!erase_step(T, row, kind, live, model, st)) return false;
    } else {
      if (!revoke_step(rng, A, world, model, st)) return false;
    }
    st.steps++;
    if (model.size() > st.max_entries) st.max_entries = model.size();
    if (model.size() > kMaxEntries) return false;
    if (!structure_ok(T) || !universe_ok(T, world, model, st)) return false;
  }
  return true;
}

int print_hashes() {
  printf("[");
  for (uint32_t c = 0; c < 4; c++) {
    uint32_t ref[kRefWords];
    for (uint32_t i = 0; i < kRefWords; i++) ref[i] = c == 0 ? 0u : (i + 1) * 0x01010101u * c + (c == 3 ? 0x80000000u : 0u);
    const uint64_t k0 = c == 0 ? 0 : 0x0706050403020100ull * c, k1 = c == 0 ? 0 : 0x0f0e0d0c0b0a0908ull ^ c;
    printf("%s{\"ref\": [", c ? ", " : "");
    for (uint32_t i = 0; i < kRefWords; i++) printf("%s%u", i ? ", " : "", ref[i]);
    printf("], \"k0\": %llu, \"k1\": %llu, \"hash\": %llu}", (unsigned long long)k0, (unsigned long long)k1,
           (unsigned long long)hash_ref(ref, k0, k1));
  }
  printf("]\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--hash")) return print_hashes();
  const uint64_t rounds = argc > 1 ? strtoull(argv[1], nullptr, 10) : 2000;
  Rng rng{argc > 2 ? strtoull(argv[2], nullptr, 10) : 1};
  Stats st;
  for (uint64_t r = 0; r < rounds; r++)
    if (!run_round(rng, st)) {
      st.failures++;
      fprintf(stderr, "round %llu failed\n", (unsigned long long)r);
      break;
    }
#define F(name) , (unsigned long long)st.name
  printf("{\"ok\": %s, \"rounds\": %llu, \"failures\": %llu, \"steps\": %llu, \"loads\": %llu, \"batches\": %llu, "
         "\"committed\": %llu, \"removals\": %llu, \"refused_absent\": %llu, \"refused_id\": %llu, "
         "\"refused_index\": %llu, \"refused_caller\": %llu, \"wrap_shifts\": %llu, \"erased_cluster_starts\": %llu, "
         "\"cluster_splits\": %llu, \"revokes\": %llu, \"revoke_rows\": %llu, \"revoke_removed\": %llu, "
         "\"adjacent_marked\": %llu, \"wrapping_clusters_repaired\": %llu, \"max_entries\": %llu, \"lookups\": %llu}\n",
         st.failures ? "false" : "true", (unsigned long long)rounds F(failures) F(steps) F(loads) F(batches) F(committed)
             F(removals) F(refused_absent) F(refused_id) F(refused_index) F(refused_caller) F(wrap_shifts)
                 F(erased_cluster_starts) F(cluster_splits) F(revokes) F(revoke_rows) F(revoke_removed)
                     F(adjacent_marked) F(wrapping_clusters_repaired) F(max_entries) F(lookups));
#undef F
  return st.failures ? 1 : 0;
}
