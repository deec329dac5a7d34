// Host check of the RSA routing geometry (corda_amd/csrc/rsa_route.hpp), built with
// ASan + UBSan by tests/test_rsa_route_check.py. The passes of rsa_route.hip are
// replayed on the host wave by wave -- the gather of the live records' (id, words, e,
// n[0]), the match, a wave's ballots, one reservation per list and wave, the ranked
// writes -- into heap buffers of exactly the sizes the layout names (modulus rows m * W
// words, scratch rsa_route_scratch_words(cap) words) and compared with a plain
// sequential partition that knows nothing of waves:
//   route[i] names a live record of class W with the row's exponent and W modulus
//     words, or kVkeyNoId exactly when none does (memcmp over the table, slot by slot);
//   the two counts are the sequential list sizes; each list, sorted, is the sequential
//     list; no position is written twice or left out; every wave's segment is ascending;
//     a row the prep decided is in neither list; the totals count every row by match;
//   the same holds when the waves reserve their ranges in a shuffled order;
//   the indexed kernels' grids (rsa_route_idx_blocks over the launch's rows) visit every
//     list position below the count exactly once, blocks wholly past it are dead;
//   the launch loop over workspace caps of 64, 128 and 4096 rows covers every row of the
//     batch exactly once with counters fresh per launch, and a launch's lists hold rows
//     of that launch only.
// Tables: 0, 1 and 64 live records; all three classes and one only; a cleared record
// whose modulus matches; the same key live twice; records equal in n[0] and e that
// differ only in the top word or only in a middle word; equal n with different e; a
// short key in a wider row.
// Usage: rsa_route_check <seed>; prints one JSON line, exit 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../corda_amd/csrc/rsa_route.hpp"

using namespace cordahip;

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static uint64_t failures = 0, cases = 0, rows_checked = 0, keyed_seen = 0, decided_seen = 0, dup_hits = 0,
                cleared_misses = 0, top_misses = 0, mid_misses = 0, exp_misses = 0, short_misses = 0, launches = 0,
                multi_launch_cases = 0, dead_blocks = 0, class_hits[3] = {0, 0, 0};
#define CHECK(c)                                                           \
  do {                                                                     \
    if (!(c)) {                                                            \
      if (failures++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
    }                                                                      \
  } while (0)

constexpr uint8_t kOkStatus = 0, kDecided = 3;

// a key: class, exponent, modulus (words above the class are zero)
struct Key {
  uint32_t words, e;
  uint32_t n[rsa::kMaxWords];
};
static Key random_key(uint32_t words, uint32_t e) {
  Key k;
  memset(&k, 0, sizeof k);
  k.words = words;
  k.e = e;
  for (uint32_t q = 0; q < words; q++) k.n[q] = (uint32_t)rng();
  k.n[0] |= 1u;
  k.n[words - 1] |= 0x80000000u;
  return k;
}

struct Table {
  std::vector<uint32_t> recs = std::vector<uint32_t>((size_t)kVkeySlots * rsa::kVkeyRecWords, 0u);
  // a live record; cleared: the record as cordahip_vkey_remove leaves it but for the
  // modulus (id 0: a zeroed record matches nothing even where its other words survive)
  void put(uint32_t slot, const Key& k, uint32_t gen, bool cleared = false) {
    uint32_t* r = &recs[(size_t)slot * rsa::kVkeyRecWords];
    memset(r, 0, rsa::kVkeyRecWords * 4);
    r[rsa::kVkeyRecIdWord] = cleared ? 0u : vkey_make_id(slot, gen);
    r[rsa::kVkeyRecEWord] = k.e;
    r[rsa::kVkeyRecWordsWord] = k.words;
    memcpy(r + rsa::kVkeyRecNWord, k.n, 4 * (size_t)k.words);
  }
};

struct Row {
  uint32_t e;
  uint8_t st;
  uint32_t n[rsa::kMaxWords];  // the first W words are the row
};
static Row row_of(const Key& k, uint8_t st = kOkStatus) {
  Row r;
  r.e = k.e;
  r.st = st;
  memcpy(r.n, k.n, sizeof r.n);
  return r;
}

// the rule stated without the header's helpers
static bool ref_slot_matches(const Table& t, uint32_t s, uint32_t W, const Row& r) {
  const uint32_t* rec = &t.recs[(size_t)s * rsa::kVkeyRecWords];
  if (rec[0] == 0u || rec[0] == 0xFFFFFFFFu || (rec[0] >> 6) == 0u) return false;
  if (rec[3] != W || rec[1] != r.e) return false;
  return memcmp(rec + 8, r.n, 4 * (size_t)W) == 0;
}
static bool ref_any(const Table& t, uint32_t W, const Row& r) {
  for (uint32_t s = 0; s < kVkeySlots; s++)
    if (ref_slot_matches(t, s, W, r)) return true;
  return false;
}
static bool ref_id_matches(const Table& t, uint32_t W, const Row& r, uint32_t id) {
  for (uint32_t s = 0; s < kVkeySlots; s++)
    if (t.recs[(size_t)s * rsa::kVkeyRecWords] == id && ref_slot_matches(t, s, W, r)) return true;
  return false;
}

// the row's modulus in a heap buffer of exactly W words: ASan sees any read past it
static uint32_t match_exact(const Table& t, uint32_t W, const Row& r) {
  std::vector<uint32_t> cand((size_t)kVkeySlots * kRsaRouteCandWords);
  const uint32_t nc = rsa_route_gather(cand.data(), t.recs.data());
  uint32_t* m = new uint32_t[W];
  memcpy(m, r.n, 4 * (size_t)W);
  const uint32_t id = rsa_route_match(W, r.e, m, cand.data(), nc, t.recs.data());
  delete[] m;
  return id;
}

// One batch of class W through the launch loop over a workspace of ws_rows rows.
// shuffle: the order in which a launch's waves reserve their ranges.
static void run_case(const Table& t, uint32_t W, const std::vector<Row>& rows, uint64_t ws_rows, bool shuffle) {
  const uint64_t n = rows.size();
  cases++;
  uint32_t* cand = new uint32_t[(size_t)kVkeySlots * kRsaRouteCandWords];  // the block's LDS
  const uint32_t ncand = rsa_route_gather(cand, t.recs.data());
  uint32_t ref_live = 0;
  for (uint32_t s = 0; s < kVkeySlots; s++) {
    const uint32_t id = t.recs[(size_t)s * rsa::kVkeyRecWords];
    ref_live += id != 0u && id != 0xFFFFFFFFu && (id >> 6) != 0u;
  }
  CHECK(ncand == ref_live);
  // the scratch follows the largest launch (runtime.cpp rsa_verify_enqueue)
  const uint64_t cap = std::min<uint64_t>(ws_rows, (n + 63) / 64 * 64);
  const uint64_t words = rsa_route_scratch_words(cap);
  uint32_t* scratch = new uint32_t[words];  // exact size: ASan sees any overrun
  memset(scratch, 0xA5, words * 4);
  uint64_t totals[2] = {0, 0};
  std::vector<uint8_t> visited(n, 0);
  uint64_t want_keyed_total = 0, want_generic_total = 0, nlaunch = 0;

  for (uint64_t lo = 0; lo < n; lo += ws_rows) {
    const uint64_t m = rsa_route_launch_rows(ws_rows, n, lo);
    CHECK(m >= 1 && m <= ws_rows && m <= cap);
    nlaunch++;
    launches++;
    // the launch's rows, exactly m * W words
    uint32_t* mod = new uint32_t[m * W];
    uint32_t* exp = new uint32_t[m];
    uint8_t* st = new uint8_t[m];
    for (uint64_t i = 0; i < m; i++) {
      memcpy(mod + i * W, rows[lo + i].n, 4 * (size_t)W);
      exp[i] = rows[lo + i].e;
      st[i] = rows[lo + i].st;
      visited[lo + i]++;
    }
    // counters fresh per launch: the lists' stale contents stay, the counts do not
    scratch[kRsaRouteCntKeyed] = scratch[kRsaRouteCntGeneric] = 0;
    uint32_t* route = scratch + rsa_route_off_route(cap);
    uint32_t* keyed = scratch + rsa_route_off_keyed(cap);
    uint32_t* generic = scratch + rsa_route_off_generic(cap);
    CHECK(rsa_route_off_generic(cap) + cap == words);

    const uint64_t blocks = (m + kRsaRouteBlock - 1) / kRsaRouteBlock;
    std::vector<uint64_t> order(blocks * 4);
    std::iota(order.begin(), order.end(), 0);
    if (shuffle)
      for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[rng() % i]);
    struct Seg {
      const uint32_t* list;
      uint64_t start, len;
    };
    std::vector<Seg> segs;
    for (uint64_t w : order) {
      const uint64_t block = w / 4;
      const uint32_t wave = (uint32_t)(w % 4);
      uint64_t mk = 0, mg = 0, lk = 0, lg = 0;
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t i = rsa_route_row(block, wave * 64 + lane);
        if (i >= m) continue;
        const uint32_t id = rsa_route_match(W, exp[i], mod + i * W, cand, ncand, t.recs.data());
        route[i] = id;
        const bool k = id != kVkeyNoId, listed = st[i] == kOkStatus;
        (k ? mk : mg) |= 1ull << lane;
        if (listed) (k ? lk : lg) |= 1ull << lane;
      }
      uint32_t sk = 0, sg = 0;  // one reservation per list
      if (lk) {
        sk = scratch[kRsaRouteCntKeyed];
        scratch[kRsaRouteCntKeyed] += (uint32_t)__builtin_popcountll(lk);
        segs.push_back({keyed, sk, (uint64_t)__builtin_popcountll(lk)});
      }
      if (lg) {
        sg = scratch[kRsaRouteCntGeneric];
        scratch[kRsaRouteCntGeneric] += (uint32_t)__builtin_popcountll(lg);
        segs.push_back({generic, sg, (uint64_t)__builtin_popcountll(lg)});
      }
      totals[0] += (uint64_t)__builtin_popcountll(mk);
      totals[1] += (uint64_t)__builtin_popcountll(mg);
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t i = (uint32_t)rsa_route_row(block, wave * 64 + lane);
        if ((lk >> lane) & 1) keyed[sk + route_rank(lk, lane)] = i;
        if ((lg >> lane) & 1) generic[sg + route_rank(lg, lane)] = i;
      }
    }

    // the plain sequential partition of this launch
    std::vector<uint32_t> want_k, want_g;
    for (uint64_t i = 0; i < m; i++) {
      const Row& r = rows[lo + i];
      const bool any = ref_any(t, W, r);
      if (any) {
        CHECK(route[i] != kVkeyNoId && ref_id_matches(t, W, r, route[i]));
        keyed_seen++;
        class_hits[W / 32 - 2]++;
        want_keyed_total++;
      } else {
        CHECK(route[i] == kVkeyNoId);
        want_generic_total++;
      }
      if (r.st != kOkStatus) {
        decided_seen++;
        continue;
      }
      (any ? want_k : want_g).push_back((uint32_t)i);
    }
    rows_checked += m;
    const uint32_t ck = scratch[kRsaRouteCntKeyed], cg = scratch[kRsaRouteCntGeneric];
    CHECK(ck == want_k.size() && cg == want_g.size());
    if (ck == want_k.size() && cg == want_g.size()) {
      for (const Seg& s : segs) CHECK(std::is_sorted(s.list + s.start, s.list + s.start + s.len));
      std::vector<uint32_t> gk(keyed, keyed + ck), gg(generic, generic + cg);
      std::sort(gk.begin(), gk.end());
      std::sort(gg.begin(), gg.end());
      CHECK(gk == want_k && gg == want_g);  // no position twice, none left out, no decided row
      // the indexed kernels: grids for m rows, the count read on the device
      for (int list = 0; list < 2; list++) {
        const uint64_t count = list ? cg : ck;
        std::vector<uint8_t> hit(count, 0);
        const uint64_t gblocks = rsa_route_idx_blocks(m);
        CHECK(gblocks * kRsaRouteGroupsPerBlock >= m);
        for (uint64_t b = 0; b < gblocks; b++) {
          if (!rsa_route_idx_block_live(b, count)) {
            dead_blocks++;
            for (uint32_t g = 0; g < (uint32_t)kRsaRouteGroupsPerBlock; g++) CHECK(rsa_route_idx_pos(b, g) >= count);
            continue;
          }
          for (uint32_t g = 0; g < (uint32_t)kRsaRouteGroupsPerBlock; g++) {
            const uint64_t j = rsa_route_idx_pos(b, g);
            if (j >= count) continue;  // stand-ins
            const uint32_t row = (list ? generic : keyed)[j];
            CHECK(row < m);
            hit[j]++;
          }
        }
        for (uint64_t j = 0; j < count; j++) CHECK(hit[j] == 1);
      }
    }
    // the header's unused words are untouched, and nothing past the launch's rows in route
    for (uint32_t j = 2; j < kRsaRouteHdrWords; j++) CHECK(scratch[j] == 0xA5A5A5A5u);
    delete[] st;
    delete[] exp;
    delete[] mod;
  }
  for (uint64_t i = 0; i < n; i++) CHECK(visited[i] == 1);
  CHECK(nlaunch == (n + ws_rows - 1) / ws_rows);
  if (nlaunch > 1) multi_launch_cases++;
  CHECK(totals[0] == want_keyed_total && totals[1] == want_generic_total && totals[0] + totals[1] == n);
  delete[] scratch;
  delete[] cand;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  // layout and the allocation's byte formula
  CHECK(kRsaRouteHdrWords == 16 && rsa_route_off_route(64) == 16 && rsa_route_off_keyed(64) == 80 &&
        rsa_route_off_generic(64) == 144 && rsa_route_scratch_words(64) * 4 == 64 + 12 * 64);
  CHECK(rsa_route_scratch_words(131072) * 4 == 64 + 12 * 131072);
  CHECK(kRsaRouteCandWords == 4 && kRsaRouteBlock == 256 && kRsaRouteGroupsPerBlock == 32);
  CHECK(rsa_route_idx_blocks(1) == 1 && rsa_route_idx_blocks(32) == 1 && rsa_route_idx_blocks(33) == 2);
  CHECK(!rsa_route_idx_block_live(0, 0) && rsa_route_idx_block_live(0, 1) && !rsa_route_idx_block_live(1, 32) &&
        rsa_route_idx_block_live(1, 33));
  CHECK(rsa_route_launch_rows(64, 130, 0) == 64 && rsa_route_launch_rows(64, 130, 64) == 64 &&
        rsa_route_launch_rows(64, 130, 128) == 2);

  // one key per class; relatives of the 96-word key K
  const Key K64 = random_key(64, 65537), K = random_key(96, 65537), K128 = random_key(128, 65537),
            U = random_key(96, 65537);
  Key TOP = K, MID = K, E3 = K, E17 = K;
  TOP.n[95] ^= 0x40000000u;  // n[0] and e equal: differs only in its top word
  MID.n[47] ^= 1u;           // ... only in a middle word
  E3.e = 3;                  // equal n, another e
  E17.e = 17;
  Key SHORT96 = K64;  // the 2048-bit key's modulus zero-padded in a 96-word row: its class stays 64
  Key SHORT128 = K64;

  std::vector<Table> tables;
  {
    Table none;  // 0 live records: a zeroed table ...
    tables.push_back(none);
    Table cleared;  // ... and one whose only matching record is cleared
    cleared.put(3, K, 5, true);
    cleared.put(9, K64, 2, true);
    tables.push_back(cleared);
    Table one;  // 1 live record (one class only), in a slot away from 0
    one.put(17, K, 1);
    tables.push_back(one);
    Table three;  // all three classes
    three.put(1, K64, 1);
    three.put(2, K, 1);
    three.put(3, K128, 1);
    tables.push_back(three);
    Table rel;  // K's relatives live, K itself only cleared
    rel.put(0, TOP, 1);
    rel.put(1, MID, 1);
    rel.put(2, E3, 1);
    rel.put(3, K, 2, true);
    rel.put(4, K64, 1);
    tables.push_back(rel);
    Table rel_k = rel;  // and with K live behind them
    rel_k.put(40, K, 3);
    tables.push_back(rel_k);
    Table dup;  // the same key live twice, a cleared copy below both
    dup.put(4, K, 9, true);
    dup.put(5, K, 2);
    dup.put(63, K, 7);
    dup.put(6, K128, 1);
    tables.push_back(dup);
    Table full;  // 64 live records over the three classes, K, K64, K128 in the last three slots
    for (uint32_t s = 0; s < kVkeySlots - 3; s++) full.put(s, random_key(64 + 32 * (s % 3), 65537), 1 + s);
    full.put(kVkeySlots - 3, K64, 3);
    full.put(kVkeySlots - 2, K, kVkeyGenMax);
    full.put(kVkeySlots - 1, K128, 3);
    tables.push_back(full);
  }

  // single-row probes of the rule, each modulus row of exactly W words
  for (const Table& t : tables) {
    const bool live = ref_any(t, 96, row_of(K));
    CHECK((match_exact(t, 96, row_of(K)) != kVkeyNoId) == live);
    if (!live) cleared_misses++;
    CHECK((match_exact(t, 96, row_of(TOP)) != kVkeyNoId) == ref_any(t, 96, row_of(TOP)));
    CHECK((match_exact(t, 96, row_of(MID)) != kVkeyNoId) == ref_any(t, 96, row_of(MID)));
    CHECK((match_exact(t, 96, row_of(E3)) != kVkeyNoId) == ref_any(t, 96, row_of(E3)));
    CHECK(match_exact(t, 96, row_of(E17)) == kVkeyNoId);
    CHECK(match_exact(t, 96, row_of(U)) == kVkeyNoId);
    if (live && !ref_any(t, 96, row_of(TOP))) top_misses++;
    if (live && !ref_any(t, 96, row_of(MID))) mid_misses++;
    if (live) exp_misses++;  // E17 is in no table
    // a short key in a wider row, and a wide key's low words in a narrower call
    CHECK(match_exact(t, 96, row_of(SHORT96)) == kVkeyNoId);
    CHECK(match_exact(t, 128, row_of(SHORT128)) == kVkeyNoId);
    CHECK((match_exact(t, 64, row_of(K64)) != kVkeyNoId) == ref_any(t, 64, row_of(K64)));
    CHECK(match_exact(t, 64, row_of(K)) == kVkeyNoId);
    if (ref_any(t, 64, row_of(K64))) short_misses++;
  }
  {
    const Table& dup = tables[6];
    const uint32_t id = match_exact(dup, 96, row_of(K));
    CHECK(id == vkey_make_id(5, 2) || id == vkey_make_id(63, 7));
    dup_hits++;
  }

  const uint64_t sizes[] = {1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 513};
  const uint64_t caps[] = {64, 128, 4096};
  for (const Table& t : tables)
    for (uint32_t W : {64u, 96u, 128u}) {
      const Key& P = W == 64 ? K64 : W == 96 ? K : K128;
      for (uint64_t n : sizes)
        for (int pat = 0; pat < 5; pat++) {
          std::vector<Row> rows(n);
          for (uint64_t i = 0; i < n; i++) {
            bool k;
            switch (pat) {
              case 0: k = true; break;                        // all on the registered key
              case 1: k = false; break;                       // none
              case 2: k = i % 2 == 0; break;                  // alternating
              case 3: k = i + 40 >= 256 && i < 256 + 40; break;  // a keyed run crossing a block edge (and launch edges)
              default: k = rng() % 3 == 0; break;
            }
            if (k) {
              rows[i] = row_of(P);
            } else if (pat == 4 && W == 96) {
              switch (rng() % 6) {
                case 0: rows[i] = row_of(TOP); break;
                case 1: rows[i] = row_of(MID); break;
                case 2: rows[i] = row_of(E3); break;
                case 3: rows[i] = row_of(SHORT96); break;
                default: rows[i] = row_of(U); break;
              }
            } else {
              rows[i] = row_of(random_key(W, 65537));
            }
            // rows the prep decided, keyed and not: every fifth row of the mixed patterns
            if (pat >= 2 && i % 5 == 3) rows[i].st = kDecided;
          }
          for (uint64_t ws : caps) {
            run_case(t, W, rows, ws, false);
            run_case(t, W, rows, ws, true);
          }
        }
    }
  printf("{\"ok\": %s, \"failures\": %llu, \"cases\": %llu, \"tables\": %zu, \"rows\": %llu, \"keyed\": %llu, "
         "\"decided\": %llu, \"class_hits\": [%llu, %llu, %llu], \"dup_hits\": %llu, \"cleared_misses\": %llu, "
         "\"top_misses\": %llu, \"mid_misses\": %llu, \"exp_misses\": %llu, \"short_misses\": %llu, "
         "\"launches\": %llu, \"multi_launch_cases\": %llu, \"dead_blocks\": %llu}\n",
         failures ? "false" : "true", (unsigned long long)failures, (unsigned long long)cases, tables.size(),
         (unsigned long long)rows_checked, (unsigned long long)keyed_seen, (unsigned long long)decided_seen,
         (unsigned long long)class_hits[0], (unsigned long long)class_hits[1], (unsigned long long)class_hits[2],
         (unsigned long long)dup_hits, (unsigned long long)cleared_misses, (unsigned long long)top_misses,
         (unsigned long long)mid_misses, (unsigned long long)exp_misses, (unsigned long long)short_misses,
         (unsigned long long)launches, (unsigned long long)multi_launch_cases, (unsigned long long)dead_blocks);
  return failures ? 1 : 0;
}
