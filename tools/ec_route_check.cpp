// Host check of the ECDSA routing geometry (corda_amd/csrc/ecdsa_route.hpp), built
// with ASan + UBSan by tests/test_ec_route_check.py. The passes of ecdsa_route.hip
// are replayed on the host wave by wave -- the gather of the live records, the
// match, the per-block class totals, the per-wave ballots, one reservation per wave
// and class, the ranked writes -- into heap buffers of exactly the sizes the layout
// names (key rows n * 65 bytes, scratch ec_route_scratch_words(n) words, perm n
// words, 14 counters), and compared with a plain sequential partition that knows
// nothing of tiles or waves:
//   route[i] names a live record of lane i's scheme one of whose point's two SEC1
//     encodings equals the lane's key bytes, or kVkeyNoId exactly when none does
//     (memcmp over the table, slot by slot, the encodings built byte by byte);
//   the seven counts are the sequential class sizes; each class's run of perm,
//     sorted, is the sequential list of that class; no position is written twice or
//     left out; every wave's segment of a run is ascending;
//   the same holds when the waves reserve their ranges in a shuffled order;
//   the generic list is perm[0 .. g), the keyed runs follow at ec_route_keyed_start;
//   the generic engine's workspace chunks (route_chunk_lanes) tile the generic list
//     exactly once for four workspace sizes, chunks wholly past the count are empty.
// Tables: 0, 1 and 64 live keys; both curves live and one curve only; a dead record
// (live word 0, and one with a zero reuse counter) whose point matches; the same
// point live twice; records with an equal first X word and different tails. Lanes:
// both encodings of a registered point, the wrong parity, another Y (the negated
// point's place), the registered bytes under the other scheme byte and under scheme 4,
// hybrid prefixes, key_len 1, 33, 64 and 65. Lane counts sit on wave, block and tile
// edges.
// Usage: ec_route_check <seed>; prints one JSON line, exit 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../corda_amd/csrc/ecdsa_route.hpp"

using namespace cordahip;

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static uint64_t failures = 0, cases = 0, lanes_checked = 0, keyed_seen = 0, keyed_k1 = 0, keyed_r1 = 0, dup_hits = 0,
                dead_misses = 0, tail_misses = 0, scheme_misses = 0, parity_misses = 0, negy_misses = 0,
                len_misses = 0, comp_hits = 0, unc_hits = 0, chunk_cases = 0, empty_chunks = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      if (failures++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
    }                                                             \
  } while (0)

// a point: plain coordinates, little-endian words (what the device converts an entry to)
struct Point {
  uint32_t x[8], y[8];
};
static Point random_point() {
  Point p;
  for (int q = 0; q < 8; q++) {
    p.x[q] = (uint32_t)rng();
    p.y[q] = (uint32_t)rng();
  }
  return p;
}

// the records of an ECDSA key table and, beside them, each slot's point
struct Table {
  std::vector<uint32_t> recs = std::vector<uint32_t>(kVkeySlots * kEcVkeyRecWords, 0u);
  std::vector<uint32_t> points = std::vector<uint32_t>(kVkeySlots * 16, 0u);
  void put(uint32_t slot, uint32_t scheme, const Point& p, uint32_t gen, uint32_t live) {
    uint32_t* r = &recs[slot * kEcVkeyRecWords];
    r[kEcVkeyRecScheme] = scheme;
    r[kEcVkeyRecId] = vkey_make_id(slot, gen);
    r[kEcVkeyRecLive] = live;
    memcpy(&points[slot * 16], p.x, 32);
    memcpy(&points[slot * 16 + 8], p.y, 32);
  }
};

struct Lane {
  uint8_t scheme, key_len;
  uint8_t key[65];
};

// the rule stated without the header's helpers
static void be32(uint8_t out[32], const uint32_t w[8]) {
  for (int b = 0; b < 32; b++) out[b] = (uint8_t)(w[7 - b / 4] >> (8 * (3 - b % 4)));
}
static bool ref_live(const uint32_t* rec) {
  return rec[kEcVkeyRecLive] == 1u && (rec[kEcVkeyRecId] >> 6) != 0u && rec[kEcVkeyRecId] != 0xFFFFFFFFu &&
         (rec[kEcVkeyRecScheme] == 2u || rec[kEcVkeyRecScheme] == 3u);
}
static bool ref_slot_matches(const Table& t, uint32_t s, const Lane& l) {
  const uint32_t* rec = &t.recs[s * kEcVkeyRecWords];
  if (!ref_live(rec) || rec[kEcVkeyRecScheme] != l.scheme) return false;
  uint8_t enc[65];
  be32(enc + 1, &t.points[s * 16]);
  be32(enc + 33, &t.points[s * 16 + 8]);
  if (l.key_len == 65) {
    enc[0] = 4;
    return memcmp(enc, l.key, 65) == 0;
  }
  if (l.key_len == 33) {
    enc[0] = (uint8_t)(2 | (enc[64] & 1));
    return memcmp(enc, l.key, 33) == 0;
  }
  return false;
}
static bool ref_any(const Table& t, const Lane& l) {
  for (uint32_t s = 0; s < kVkeySlots; s++)
    if (ref_slot_matches(t, s, l)) return true;
  return false;
}
static bool ref_id_matches(const Table& t, const Lane& l, uint32_t id) {
  for (uint32_t s = 0; s < kVkeySlots; s++)
    if (t.recs[s * kEcVkeyRecWords + kEcVkeyRecId] == id && ref_slot_matches(t, s, l)) return true;
  return false;
}
static int ref_class(const Lane& l, bool keyed) {
  if (keyed) return l.scheme == 2 ? 5 : 6;
  if (l.scheme == 2) return l.key_len == 33 ? 1 : 0;
  if (l.scheme == 3) return l.key_len == 33 ? 3 : 2;
  return 4;
}

static Lane lane_unc(uint8_t scheme, const Point& p) {
  Lane l;
  l.scheme = scheme;
  l.key_len = 65;
  l.key[0] = 4;
  be32(l.key + 1, p.x);
  be32(l.key + 33, p.y);
  return l;
}
static Lane lane_comp(uint8_t scheme, const Point& p, bool wrong_parity = false) {
  Lane l = lane_unc(scheme, p);
  l.key_len = 33;
  l.key[0] = (uint8_t)(2 | ((p.y[0] & 1) ^ (wrong_parity ? 1 : 0)));
  return l;
}

// the lane's key row in a heap buffer of exactly key_len bytes: ASan sees any read past it
static uint32_t match_exact(const Lane& l, const uint32_t* gathered, uint32_t nlive) {
  uint8_t* row = new uint8_t[l.key_len ? l.key_len : 1];
  memcpy(row, l.key, l.key_len);
  const uint32_t id = ec_route_match(l.scheme, l.key_len, row, gathered, nlive);
  delete[] row;
  return id;
}

// One replay of the passes. shuffle: the order in which the waves reserve their ranges.
static void run_case(const Table& t, const std::vector<Lane>& lanes, bool shuffle) {
  const uint64_t n = lanes.size();
  cases++;
  uint8_t* scheme = new uint8_t[n];
  uint8_t* key_len = new uint8_t[n];
  uint8_t* keys = new uint8_t[n * 65];
  for (uint64_t i = 0; i < n; i++) {
    scheme[i] = lanes[i].scheme;
    key_len[i] = lanes[i].key_len;
    memcpy(keys + i * 65, lanes[i].key, 65);
  }
  const uint64_t words = ec_route_scratch_words(n);
  uint32_t* scratch = new uint32_t[words];  // exact size: ASan sees any overrun
  memset(scratch, 0xA5, words * 4);
  uint32_t* perm = new uint32_t[n];
  memset(perm, 0xA5, n * 4);
  uint32_t counters[2 * kEcRouteClasses] = {};
  uint32_t* counts = counters;
  uint32_t* cursors = counters + kEcRouteClasses;
  uint64_t totals[2] = {0, 0};
  uint32_t* route = scratch + ec_route_off_route();

  // gather
  const uint32_t nlive = ec_route_gather(scratch + kEcRouteRecBase, t.recs.data(), t.points.data());
  scratch[kEcRouteCntLive] = nlive;
  uint32_t ref_nlive = 0;
  for (uint32_t s = 0; s < kVkeySlots; s++) ref_nlive += ref_live(&t.recs[s * kEcVkeyRecWords]);
  CHECK(nlive == ref_nlive);
  const uint32_t* gathered = scratch + kEcRouteRecBase;

  // route: a block's class totals, one add per class
  const uint64_t blocks = (n + kEcRouteTile - 1) / kEcRouteTile;
  for (uint64_t block = 0; block < blocks; block++) {
    uint32_t part[kEcRouteClasses][4] = {};
    for (uint32_t wave = 0; wave < 4; wave++)
      for (int it = 0; it < kEcRouteIter; it++)
        for (uint32_t lane = 0; lane < 64; lane++) {
          const uint64_t i = ec_route_tile_lane(block, it, wave * 64 + lane);
          if (i >= n) continue;
          const uint32_t id = ec_route_match(scheme[i], key_len[i], keys + i * 65, gathered, nlive);
          route[i] = id;
          part[ec_route_class(scheme[i], key_len[i], id)][wave]++;
        }
    for (int k = 0; k < kEcRouteClasses; k++) {
      const uint32_t tot = part[k][0] + part[k][1] + part[k][2] + part[k][3];
      counts[k] += tot;
      totals[k < kEcRouteGenericClasses ? 1 : 0] += tot;
    }
  }

  // scatter: a wave's ballots, one reservation per class, ranked writes
  std::vector<uint64_t> order(blocks * 4);
  std::iota(order.begin(), order.end(), 0);
  if (shuffle)
    for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[rng() % i]);
  struct Seg {
    uint64_t start, len;
  };
  std::vector<Seg> segs;
  for (uint64_t w : order) {
    const uint64_t block = w / 4;
    const uint32_t wave = (uint32_t)(w % 4);
    uint64_t bal[kEcRouteIter][kEcRouteClasses];
    uint32_t tot[kEcRouteClasses] = {};
    for (int it = 0; it < kEcRouteIter; it++) {
      for (int k = 0; k < kEcRouteClasses; k++) bal[it][k] = 0;
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t i = ec_route_tile_lane(block, it, wave * 64 + lane);
        if (i < n) bal[it][ec_route_class(scheme[i], key_len[i], route[i])] |= 1ull << lane;
      }
      for (int k = 0; k < kEcRouteClasses; k++) tot[k] += (uint32_t)__builtin_popcountll(bal[it][k]);
    }
    uint64_t start[kEcRouteClasses], base = 0;
    for (int k = 0; k < kEcRouteClasses; k++) {
      uint32_t s0 = 0;
      if (tot[k]) {
        s0 = cursors[k];
        cursors[k] += tot[k];
      }
      start[k] = s0 + base;
      base += counts[k];
      if (tot[k]) segs.push_back({start[k], tot[k]});
    }
    for (int it = 0; it < kEcRouteIter; it++)
      for (int k = 0; k < kEcRouteClasses; k++) {
        for (uint32_t lane = 0; lane < 64; lane++)
          if ((bal[it][k] >> lane) & 1)
            perm[start[k] + route_rank(bal[it][k], lane)] = (uint32_t)ec_route_tile_lane(block, it, wave * 64 + lane);
        start[k] += (uint32_t)__builtin_popcountll(bal[it][k]);
      }
  }

  // the plain sequential partition
  std::vector<uint32_t> want[kEcRouteClasses];
  for (uint64_t i = 0; i < n; i++) {
    const bool any = ref_any(t, lanes[i]);
    if (any) {
      CHECK(route[i] != kVkeyNoId && ref_id_matches(t, lanes[i], route[i]));
      keyed_seen++;
      (lanes[i].scheme == 2 ? keyed_k1 : keyed_r1)++;
    } else {
      CHECK(route[i] == kVkeyNoId);
    }
    want[ref_class(lanes[i], any)].push_back((uint32_t)i);
  }
  lanes_checked += n;
  bool counts_ok = true;
  uint64_t keyed_total = 0, generic_total = 0;
  for (int k = 0; k < kEcRouteClasses; k++) {
    CHECK(counts[k] == want[k].size() && cursors[k] == want[k].size());
    counts_ok = counts_ok && counts[k] == want[k].size();
    (k < 5 ? generic_total : keyed_total) += want[k].size();
  }
  CHECK(totals[0] == keyed_total && totals[1] == generic_total && keyed_total + generic_total == n);
  if (counts_ok) {
    for (const Seg& s : segs) CHECK(std::is_sorted(perm + s.start, perm + s.start + s.len));
    uint64_t at = 0;
    for (int k = 0; k < kEcRouteClasses; k++) {
      if (k == 5) CHECK(at == ec_route_generic_count(counts) && at == ec_route_keyed_start(counts, 2));
      if (k == 6) CHECK(at == ec_route_keyed_start(counts, 3));
      std::vector<uint32_t> got(perm + at, perm + at + want[k].size());
      std::sort(got.begin(), got.end());
      CHECK(got == want[k]);  // equal as sorted lists of equal length: no position twice, none left out
      at += want[k].size();
    }
    CHECK(at == n);
    CHECK(ec_route_keyed_count(counts, 2) == want[5].size() && ec_route_keyed_count(counts, 3) == want[6].size());
    // the header's unused words and the records past the live ones are untouched
    for (uint32_t j = 1; j < kEcRouteRecBase; j++) CHECK(scratch[j] == 0xA5A5A5A5u);
    for (uint32_t j = kEcRouteRecBase + nlive * kEcRouteRecWords; j < kEcRouteHdrWords; j++)
      CHECK(scratch[j] == 0xA5A5A5A5u);
    // the generic engine's workspace chunks tile the generic list exactly once
    const uint64_t count = ec_route_generic_count(counts);
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
  delete[] perm;
  delete[] scratch;
  delete[] keys;
  delete[] key_len;
  delete[] scheme;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  // layout and the allocation's byte formula
  CHECK(kEcRouteHdrWords == 16 + 64 * 18 && ec_route_off_route() == kEcRouteHdrWords);
  CHECK(ec_route_scratch_words(route_scratch_cap_lanes(1)) * 4 == 4672 + 4 * 65536);
  CHECK(ec_route_scratch_words(route_scratch_cap_lanes(65537)) * 4 == 4672 + 4 * 131072);
  CHECK(kEcRouteClasses == 7 && kEcRouteTile == 4096);
  for (int s = 0; s < 6; s++)
    for (int kl : {1, 33, 64, 65}) {
      const int g = ec_route_generic_class((uint8_t)s, (uint8_t)kl);
      CHECK(g == (s == 2 ? (kl == 33 ? 1 : 0) : s == 3 ? (kl == 33 ? 3 : 2) : 4));
      CHECK(ec_route_class((uint8_t)s, (uint8_t)kl, kVkeyNoId) == g);
    }
  CHECK(ec_route_class(2, 65, 7) == 5 && ec_route_class(2, 33, 7) == 5 && ec_route_class(3, 65, 7) == 6 &&
        ec_route_class(3, 33, 7) == 6);

  const Point K = random_point(), R = random_point(), U = random_point();
  // tails: K's first X word (the most significant: bytes 1..4 of the key) with another tail
  Point T1 = K, T7 = K, NY = K;
  T1.x[6] ^= 1u;          // differs in the second word the match reads
  T7.x[0] ^= 0x80u;       // differs in the last
  NY.y[0] ^= 0x10u;       // K's X with another Y of the same parity: the uncompressed bytes differ,
  Point NYP = K;          // the compressed bytes do not;
  NYP.y[0] ^= 0x11u;      // and one of the other parity (where the negated point sits)

  std::vector<Table> tables;
  {
    Table none;  // 0 live keys: a zeroed table ...
    tables.push_back(none);
    Table dead;  // ... and one whose only matching records are dead
    dead.put(3, 2, K, 5, 0);   // removed: live word cleared
    dead.put(9, 2, K, 0, 1);   // a zero reuse counter is never issued
    dead.put(11, 0, K, 4, 1);  // no ECDSA scheme: an Ed25519 slot's (zeroed) record never looks like this, but still
    tables.push_back(dead);
    Table one;  // 1 live key (secp256k1 only), in a slot away from 0
    one.put(17, 2, K, 1, 1);
    tables.push_back(one);
    Table one_r1;  // P-256 only, the same point's bytes
    one_r1.put(30, 3, K, 2, 1);
    tables.push_back(one_r1);
    Table both;  // both curves live; K under 2, R under 3
    both.put(1, 2, K, 1, 1);
    both.put(2, 3, R, 1, 1);
    tables.push_back(both);
    Table tails;  // K's relatives live, K itself only dead
    tails.put(0, 2, T1, 1, 1);
    tails.put(1, 2, T7, 1, 1);
    tails.put(2, 2, K, 2, 0);
    tails.put(3, 3, R, 2, 1);
    tables.push_back(tails);
    Table tails_k = tails;  // and with K live behind them
    tails_k.put(40, 2, K, 3, 1);
    tables.push_back(tails_k);
    Table dup;  // the same point live in two slots, a dead copy below both
    dup.put(4, 2, K, 9, 0);
    dup.put(5, 2, K, 2, 1);
    dup.put(63, 2, K, 7, 1);
    dup.put(6, 3, R, 1, 1);
    tables.push_back(dup);
    Table full;  // 64 live keys, alternating curves, K and R in the last two slots
    for (uint32_t s = 0; s < kVkeySlots - 2; s++) full.put(s, 2 + (s & 1), random_point(), 1 + s, 1);
    full.put(kVkeySlots - 2, 2, K, kVkeyGenMax, 1);
    full.put(kVkeySlots - 1, 3, R, 3, 1);
    tables.push_back(full);
  }
  // single-lane probes of the rule, each key row of exactly key_len bytes
  for (const Table& t : tables) {
    std::vector<uint32_t> g(kVkeySlots * kEcRouteRecWords);
    const uint32_t nl = ec_route_gather(g.data(), t.recs.data(), t.points.data());
    for (uint8_t sch : {(uint8_t)2, (uint8_t)3}) {
      const Lane unc = lane_unc(sch, K), comp = lane_comp(sch, K);
      const bool live = ref_any(t, unc);
      CHECK(ref_any(t, comp) == live);
      CHECK((match_exact(unc, g.data(), nl) != kVkeyNoId) == live);
      CHECK((match_exact(comp, g.data(), nl) != kVkeyNoId) == live);
      if (live) unc_hits++, comp_hits++;
      else dead_misses++;
      // the same bytes under the other scheme byte, and under no ECDSA scheme
      Lane other = unc;
      other.scheme = (uint8_t)(5 - sch);
      CHECK((match_exact(other, g.data(), nl) != kVkeyNoId) == ref_any(t, other));
      if (live && !ref_any(t, other)) scheme_misses++;
      for (uint8_t s4 : {(uint8_t)0, (uint8_t)1, (uint8_t)4, (uint8_t)255}) {
        Lane o = unc;
        o.scheme = s4;
        CHECK(match_exact(o, g.data(), nl) == kVkeyNoId);
      }
      // wrong parity; another Y (same and other parity); hybrid prefixes
      CHECK(match_exact(lane_comp(sch, K, true), g.data(), nl) == kVkeyNoId);
      if (live) parity_misses++;
      CHECK(match_exact(lane_unc(sch, NY), g.data(), nl) == kVkeyNoId);
      CHECK(match_exact(lane_unc(sch, NYP), g.data(), nl) == kVkeyNoId);
      CHECK(match_exact(lane_comp(sch, NYP), g.data(), nl) == kVkeyNoId);
      CHECK((match_exact(lane_comp(sch, NY), g.data(), nl) != kVkeyNoId) == live);  // the same compressed bytes
      if (live) negy_misses++;
      for (uint8_t pre : {(uint8_t)0, (uint8_t)6, (uint8_t)7, (uint8_t)5}) {
        Lane h = unc;
        h.key[0] = pre;
        CHECK(match_exact(h, g.data(), nl) == kVkeyNoId);
      }
      Lane c4 = comp;
      c4.key[0] = 4;
      CHECK(match_exact(c4, g.data(), nl) == kVkeyNoId);
      Lane u2 = unc;
      u2.key[0] = (uint8_t)(2 | (K.y[0] & 1));
      CHECK(match_exact(u2, g.data(), nl) == kVkeyNoId);
      // other lengths: the row holds key_len bytes and not one is read
      for (uint8_t kl : {(uint8_t)0, (uint8_t)1, (uint8_t)32, (uint8_t)34, (uint8_t)64, (uint8_t)66, (uint8_t)255}) {
        Lane l = unc;
        l.key_len = kl > 65 ? 65 : kl;  // the row itself
        uint8_t* row = new uint8_t[l.key_len ? l.key_len : 1];
        memcpy(row, l.key, l.key_len);
        CHECK(ec_route_match(sch, kl, row, g.data(), nl) == kVkeyNoId);
        delete[] row;
        len_misses++;
      }
      if (!ref_any(t, lane_unc(sch, T7))) {
        CHECK(match_exact(lane_unc(sch, T7), g.data(), nl) == kVkeyNoId);
        CHECK(match_exact(lane_comp(sch, T1), g.data(), nl) == kVkeyNoId || ref_any(t, lane_comp(sch, T1)));
        tail_misses++;
      }
    }
  }
  {
    std::vector<uint32_t> g(kVkeySlots * kEcRouteRecWords);
    const Table& dup = tables[7];
    const uint32_t nl = ec_route_gather(g.data(), dup.recs.data(), dup.points.data());
    const uint32_t id = match_exact(lane_unc(2, K), g.data(), nl);
    CHECK(nl == 3 && (id == vkey_make_id(5, 2) || id == vkey_make_id(63, 7)));
    dup_hits++;
  }

  const uint64_t sizes[] = {1, 63, 64, 65, 255, 256, 257, 5 * 64 + 37, (uint64_t)kEcRouteTile - 1, kEcRouteTile,
                            (uint64_t)kEcRouteTile + 1, 2 * (uint64_t)kEcRouteTile + 65};
  for (const Table& t : tables)
    for (uint64_t n : sizes)
      for (int pat = 0; pat < 6; pat++) {
        std::vector<Lane> lanes(n);
        for (uint64_t i = 0; i < n; i++) {
          bool k;
          switch (pat) {
            case 0: k = true; break;            // all registered points
            case 1: k = false; break;           // none
            case 2: k = i % 2 == 0; break;      // alternating
            case 3: k = i == n - 1; break;      // only the last lane
            case 4: k = i % 64 == 63 || i % 256 == 0; break;  // wave and block edges
            default: k = rng() % 3 == 0; break;
          }
          const uint8_t sch = (uint8_t)(2 + (i & 1));  // curves alternate inside waves
          const Point& P = sch == 2 ? K : R;
          const bool comp = (i >> 1) & 1;
          if (k) {
            lanes[i] = comp ? lane_comp(sch, P) : lane_unc(sch, P);
          } else if (pat == 5) {
            switch (rng() % 10) {
              case 0: lanes[i] = lane_comp(sch, P, true); break;
              case 1: lanes[i] = lane_unc(sch, sch == 2 ? NYP : U); break;
              case 2: lanes[i] = lane_unc(sch, rng() & 1 ? T1 : T7); break;
              case 3: lanes[i] = lane_unc((uint8_t)(5 - sch), P); break;  // the bytes under the other scheme byte
              case 4: lanes[i] = lane_unc(4, P); break;                   // class "other"
              case 5:
                lanes[i] = lane_unc(sch, P);
                lanes[i].key_len = rng() & 1 ? 64 : 1;
                break;
              case 6:
                lanes[i] = lane_unc(sch, P);
                lanes[i].key[0] = 6;
                break;
              default: lanes[i] = comp ? lane_comp(sch, U) : lane_unc(sch, U); break;
            }
          } else {
            lanes[i] = comp ? lane_comp(sch, U) : lane_unc(sch, U);
          }
        }
        run_case(t, lanes, false);
        run_case(t, lanes, true);
      }
  printf("{\"ok\": %s, \"failures\": %llu, \"cases\": %llu, \"tables\": %zu, \"lanes\": %llu, \"keyed\": %llu, "
         "\"keyed_k1\": %llu, \"keyed_r1\": %llu, \"dup_hits\": %llu, \"dead_misses\": %llu, \"tail_misses\": %llu, "
         "\"scheme_misses\": %llu, \"parity_misses\": %llu, \"negy_misses\": %llu, \"len_misses\": %llu, "
         "\"unc_hits\": %llu, \"comp_hits\": %llu, \"chunk_cases\": %llu, \"empty_chunks\": %llu}\n",
         failures ? "false" : "true", (unsigned long long)failures, (unsigned long long)cases, tables.size(),
         (unsigned long long)lanes_checked, (unsigned long long)keyed_seen, (unsigned long long)keyed_k1,
         (unsigned long long)keyed_r1, (unsigned long long)dup_hits, (unsigned long long)dead_misses,
         (unsigned long long)tail_misses, (unsigned long long)scheme_misses, (unsigned long long)parity_misses,
         (unsigned long long)negy_misses, (unsigned long long)len_misses, (unsigned long long)unc_hits,
         (unsigned long long)comp_hits, (unsigned long long)chunk_cases, (unsigned long long)empty_chunks);
  return failures ? 1 : 0;
}
