// Host check of the Ed25519 routing geometry (corda_amd/csrc/ed25519_route.hpp),
// built with ASan + UBSan by tests/test_ed_route_check.py. The partition pass of
// ed25519_route.hip is replayed on the host wave by wave -- the gather of the live
// records, the match, the per-wave ballots, one reservation per wave and list, the
// ranked writes -- into a heap scratch of exactly route_scratch_words(n) words, and
// compared with a plain sequential partition that knows nothing of tiles or waves:
//   route[i] names a live record whose 32 bytes equal lane i's key, or kVkeyNoId
//     exactly when no live record does (memcmp over the table, slot by slot);
//   the keyed list, sorted, is the sequential list of keyed lanes, the generic list
//     likewise; both counts match; no list position is written twice or left out;
//   every wave's segment of a list is ascending;
//   the same holds when the waves reserve their ranges in a shuffled order;
//   the generic engine's workspace chunks (route_chunk_lanes) tile the generic list
//     exactly once for chunk sizes from 64 lanes up, and chunks past the count are empty.
// The capacity rule of the allocation (route_scratch_cap_lanes) is checked at its floor,
// at a power of two and one past it, and at the cap.
// Tables: 0, 1 and 64 live keys; records with equal first words and different tails;
// a dead record (live word 0, and one with a zero reuse counter) whose bytes match; the
// same bytes live in two slots. Lane counts sit on wave, block and tile edges.
// Usage: ed_route_check <seed>; prints one JSON line, exit 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../corda_amd/csrc/ed25519_route.hpp"

using namespace cordahip;

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static uint64_t failures = 0, cases = 0, lanes_checked = 0, keyed_seen = 0, dup_hits = 0, dead_misses = 0,
                tail_misses = 0, chunk_cases = 0, empty_chunks = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      if (failures++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
    }                                                             \
  } while (0)

struct Key {
  uint32_t w[8];
};
static Key random_key() {
  Key k;
  for (int q = 0; q < 8; q += 2) {
    const uint64_t r = rng();
    k.w[q] = (uint32_t)r;
    k.w[q + 1] = (uint32_t)(r >> 32);
  }
  return k;
}

// the records of a key table: kVkeySlots x kVkeyRecWords words, zeroed
struct Table {
  std::vector<uint32_t> recs = std::vector<uint32_t>(kVkeySlots * kVkeyRecWords, 0u);
  void put(uint32_t slot, const Key& k, uint32_t gen, uint32_t live) {
    uint32_t* r = &recs[slot * kVkeyRecWords];
    memcpy(r + kVkeyRecAbyte, k.w, 32);
    r[kVkeyRecId] = vkey_make_id(slot, gen);
    r[kVkeyRecLive] = live;
  }
};

// the rule stated without the header's helpers
static bool ref_live(const uint32_t* rec) { return rec[kVkeyRecLive] == 1u && (rec[kVkeyRecId] >> 6) != 0u && rec[kVkeyRecId] != 0xFFFFFFFFu; }
static bool ref_matches(const Table& t, const Key& k, uint32_t id) {  // id: a live record with k's bytes
  for (uint32_t s = 0; s < kVkeySlots; s++) {
    const uint32_t* rec = &t.recs[s * kVkeyRecWords];
    if (ref_live(rec) && rec[kVkeyRecId] == id && memcmp(rec + kVkeyRecAbyte, k.w, 32) == 0) return true;
  }
  return false;
}
static bool ref_any(const Table& t, const Key& k) {
  for (uint32_t s = 0; s < kVkeySlots; s++) {
    const uint32_t* rec = &t.recs[s * kVkeyRecWords];
    if (ref_live(rec) && memcmp(rec + kVkeyRecAbyte, k.w, 32) == 0) return true;
  }
  return false;
}

// One replay of the pass. shuffle: the order in which the waves reserve their ranges.
static void run_case(const Table& t, const std::vector<Key>& keys, bool shuffle) {
  const uint64_t n = keys.size();
  cases++;
  uint32_t* scratch = new uint32_t[route_scratch_words(n)];  // exact size: ASan sees any overrun
  memset(scratch, 0xA5, route_scratch_words(n) * 4);
  scratch[kRouteCntKeyed] = scratch[kRouteCntGeneric] = 0;
  uint32_t* route = scratch + route_off_route(n);
  uint32_t* keyed = scratch + route_off_keyed(n);
  uint32_t* generic = scratch + route_off_generic(n);
  std::vector<uint32_t> gathered(kVkeySlots * kRouteRecWords);
  const uint32_t nlive = route_gather(gathered.data(), t.recs.data());
  uint32_t ref_nlive = 0;
  for (uint32_t s = 0; s < kVkeySlots; s++) ref_nlive += ref_live(&t.recs[s * kVkeyRecWords]);
  CHECK(nlive == ref_nlive);

  const uint64_t blocks = (n + kRouteTile - 1) / kRouteTile;
  std::vector<uint64_t> order(blocks * 4);
  std::iota(order.begin(), order.end(), 0);
  if (shuffle)
    for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[rng() % i]);
  struct Seg {
    uint32_t start, len;
  };
  std::vector<Seg> ksegs, gsegs;
  for (uint64_t w : order) {
    const uint64_t block = w / 4;
    const uint32_t wave = (uint32_t)(w % 4);
    uint32_t id[kRouteIter][64];
    uint64_t bk[kRouteIter], bg[kRouteIter];
    uint32_t nk = 0, ng = 0;
    for (int it = 0; it < kRouteIter; it++) {
      bk[it] = bg[it] = 0;
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t i = route_tile_lane(block, it, wave * 64 + lane);
        id[it][lane] = kVkeyNoId;
        if (i < n) {
          id[it][lane] = route_match(keys[i].w, gathered.data(), nlive);
          route[i] = id[it][lane];
          (id[it][lane] != kVkeyNoId ? bk[it] : bg[it]) |= 1ull << lane;
        }
      }
      nk += (uint32_t)__builtin_popcountll(bk[it]);
      ng += (uint32_t)__builtin_popcountll(bg[it]);
    }
    uint32_t sk = scratch[kRouteCntKeyed], sg = scratch[kRouteCntGeneric];  // the wave's two atomics
    scratch[kRouteCntKeyed] += nk;
    scratch[kRouteCntGeneric] += ng;
    if (nk) ksegs.push_back({sk, nk});
    if (ng) gsegs.push_back({sg, ng});
    for (int it = 0; it < kRouteIter; it++) {
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t i = route_tile_lane(block, it, wave * 64 + lane);
        if ((bk[it] >> lane) & 1) keyed[sk + route_rank(bk[it], lane)] = (uint32_t)i;
        if ((bg[it] >> lane) & 1) generic[sg + route_rank(bg[it], lane)] = (uint32_t)i;
      }
      sk += (uint32_t)__builtin_popcountll(bk[it]);
      sg += (uint32_t)__builtin_popcountll(bg[it]);
    }
  }

  // the plain sequential partition
  std::vector<uint32_t> want_k, want_g;
  for (uint64_t i = 0; i < n; i++) {
    const bool any = ref_any(t, keys[i]);
    if (any) {
      CHECK(route[i] != kVkeyNoId && ref_matches(t, keys[i], route[i]));
      want_k.push_back((uint32_t)i);
    } else {
      CHECK(route[i] == kVkeyNoId);
      want_g.push_back((uint32_t)i);
    }
  }
  lanes_checked += n;
  keyed_seen += want_k.size();
  CHECK(scratch[kRouteCntKeyed] == want_k.size());
  CHECK(scratch[kRouteCntGeneric] == want_g.size());
  if (scratch[kRouteCntKeyed] == want_k.size() && scratch[kRouteCntGeneric] == want_g.size()) {
    for (const Seg& s : ksegs) CHECK(std::is_sorted(keyed + s.start, keyed + s.start + s.len));
    for (const Seg& s : gsegs) CHECK(std::is_sorted(generic + s.start, generic + s.start + s.len));
    std::vector<uint32_t> got_k(keyed, keyed + want_k.size()), got_g(generic, generic + want_g.size());
    std::sort(got_k.begin(), got_k.end());
    std::sort(got_g.begin(), got_g.end());
    CHECK(got_k == want_k);  // equal as sorted lists of equal length: no position twice, none left out
    CHECK(got_g == want_g);
    if (!shuffle) {  // waves in order: a wave's first stride of a tile's first wave leads its list
      if (!want_k.empty() && want_k[0] < 64) CHECK(keyed[0] == want_k[0]);
      if (!want_g.empty() && want_g[0] < 64) CHECK(generic[0] == want_g[0]);
    }
    // words past a list's count and the header's unused words are untouched
    for (uint64_t j = want_k.size(); j < n; j++) CHECK(keyed[j] == 0xA5A5A5A5u);
    for (uint64_t j = want_g.size(); j < n; j++) CHECK(generic[j] == 0xA5A5A5A5u);
    for (uint32_t j = 2; j < kRouteHdrWords; j++) CHECK(scratch[j] == 0xA5A5A5A5u);
    // the generic engine's workspace chunks tile the generic list exactly once
    const uint64_t count = want_g.size();
    for (uint64_t ws : {(uint64_t)64, (uint64_t)128, (uint64_t)320, (uint64_t)4096}) {
      std::vector<uint8_t> hit(count, 0);
      for (uint64_t base = 0; base < n; base += ws) {  // the host's loop: it knows n, not count
        const uint64_t m = n - base < ws ? n - base : ws;
        const uint64_t mm = route_chunk_lanes(count, base, m);
        CHECK(mm <= m);
        if (mm == 0) empty_chunks++;
        for (uint64_t li = 0; li < mm; li++) {
          CHECK(base + li < count);
          if (base + li < count) hit[base + li]++;
        }
      }
      for (uint64_t j = 0; j < count; j++) CHECK(hit[j] == 1);
      chunk_cases++;
    }
  }
  delete[] scratch;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  // layout: the arrays do not overlap and end at the scratch's end
  for (uint64_t n : {(uint64_t)1, (uint64_t)64, (uint64_t)0xFFFFFFFFull}) {
    CHECK(route_off_route(n) == kRouteHdrWords);
    CHECK(route_off_keyed(n) == route_off_route(n) + n);
    CHECK(route_off_generic(n) == route_off_keyed(n) + n);
    CHECK(route_scratch_words(n) == route_off_generic(n) + n);
  }
  // the allocation's capacity: powers of two from the floor, never below n, capped
  CHECK(route_scratch_cap_lanes(0) == kRouteMinLanes && route_scratch_cap_lanes(1) == kRouteMinLanes &&
        route_scratch_cap_lanes(kRouteMinLanes) == kRouteMinLanes &&
        route_scratch_cap_lanes(kRouteMinLanes + 1) == 2 * kRouteMinLanes &&
        route_scratch_cap_lanes((1ull << 31) + 1) == kRouteMaxLanes && route_scratch_cap_lanes(kRouteMaxLanes) == kRouteMaxLanes);
  for (uint64_t n = 1; n <= kRouteMaxLanes; n = n * 3 + 1) CHECK(route_scratch_cap_lanes(n) >= n);
  CHECK(route_rank(~0ull, 0) == 0 && route_rank(~0ull, 63) == 63 && route_rank(1ull << 63, 63) == 0 &&
        route_rank(0x8000000000000001ull, 63) == 1);
  CHECK(route_chunk_lanes(0, 0, 64) == 0 && route_chunk_lanes(64, 64, 64) == 0 && route_chunk_lanes(65, 64, 64) == 1 &&
        route_chunk_lanes(1000, 0, 64) == 64);

  const Key K = random_key(), U = random_key();
  // tails: same first word as K (and the same first seven), another last word
  Key T1 = K, T7 = K;
  T1.w[1] ^= 1u;
  T7.w[7] ^= 0x80000000u;

  std::vector<Table> tables;
  {
    Table none;  // 0 live keys: a zeroed table ...
    tables.push_back(none);
    Table dead;  // ... and one whose only matching records are dead
    dead.put(3, K, 5, 0);  // removed: live word cleared
    dead.put(9, K, 0, 1);  // a zero reuse counter is never issued
    tables.push_back(dead);
    Table one;  // 1 live key, in a slot away from 0
    one.put(17, K, 1, 1);
    tables.push_back(one);
    Table tails;  // K's relatives live, K itself only dead
    tails.put(0, T1, 1, 1);
    tails.put(1, T7, 1, 1);
    tails.put(2, K, 2, 0);
    tables.push_back(tails);
    Table tails_k = tails;  // and with K live behind them
    tails_k.put(40, K, 3, 1);
    tables.push_back(tails_k);
    Table dup;  // the same bytes live in two slots, a dead copy below both
    dup.put(4, K, 9, 0);
    dup.put(5, K, 2, 1);
    dup.put(63, K, 7, 1);
    tables.push_back(dup);
    Table full;  // 64 live keys, K in the last slot
    for (uint32_t s = 0; s < kVkeySlots - 1; s++) full.put(s, random_key(), 1 + s, 1);
    full.put(kVkeySlots - 1, K, kVkeyGenMax, 1);
    tables.push_back(full);
  }
  // single-lane probes of the rule
  for (const Table& t : tables) {
    std::vector<uint32_t> g(kVkeySlots * kRouteRecWords);
    const uint32_t nl = route_gather(g.data(), t.recs.data());
    const bool k_live = ref_any(t, K);
    CHECK((route_match(K.w, g.data(), nl) != kVkeyNoId) == k_live);
    if (!k_live) dead_misses++;
    CHECK(route_match(U.w, g.data(), nl) == kVkeyNoId);
    if (!ref_any(t, T7)) {
      CHECK(route_match(T7.w, g.data(), nl) == kVkeyNoId);
      tail_misses++;
    }
  }
  {
    std::vector<uint32_t> g(kVkeySlots * kRouteRecWords);
    const uint32_t nl = route_gather(g.data(), tables[5].recs.data());
    const uint32_t id = route_match(K.w, g.data(), nl);
    CHECK(nl == 2 && (id == vkey_make_id(5, 2) || id == vkey_make_id(63, 7)));
    dup_hits++;
  }

  const uint64_t sizes[] = {1, 63, 64, 65, 255, 256, 257, 5 * 64 + 37, (uint64_t)kRouteTile - 1, kRouteTile,
                            (uint64_t)kRouteTile + 1, 3 * (uint64_t)kRouteTile + 65};
  for (const Table& t : tables)
    for (uint64_t n : sizes)
      for (int pat = 0; pat < 6; pat++) {
        std::vector<Key> keys(n);
        for (uint64_t i = 0; i < n; i++) {
          bool k;
          switch (pat) {
            case 0: k = true; break;            // all K
            case 1: k = false; break;           // all U
            case 2: k = i % 2 == 0; break;      // alternating
            case 3: k = i == n - 1; break;      // K only in the last lane
            case 4: k = i % 64 == 63 || i % 256 == 0; break;  // wave and block edges
            default: k = rng() % 3 == 0; break;
          }
          keys[i] = k ? K : (pat == 5 && rng() % 4 == 0 ? (rng() & 1 ? T1 : T7) : U);
        }
        run_case(t, keys, false);
        run_case(t, keys, true);
      }
  printf("{\"ok\": %s, \"failures\": %llu, \"cases\": %llu, \"tables\": %zu, \"lanes\": %llu, \"keyed\": %llu, "
         "\"dup_hits\": %llu, \"dead_misses\": %llu, \"tail_misses\": %llu, \"chunk_cases\": %llu, "
         "\"empty_chunks\": %llu}\n",
         failures ? "false" : "true", (unsigned long long)failures, (unsigned long long)cases, tables.size(),
         (unsigned long long)lanes_checked, (unsigned long long)keyed_seen, (unsigned long long)dup_hits,
         (unsigned long long)dead_misses, (unsigned long long)tail_misses, (unsigned long long)chunk_cases,
         (unsigned long long)empty_chunks);
  return failures ? 1 : 0;
}
