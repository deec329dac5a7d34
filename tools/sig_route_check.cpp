// Host check of the counted route passes (K24: ed25519_route.hip, ecdsa_route.hip and
// rsa_route.hip with a row count read from device memory), built with ASan + UBSan by
// tests/test_sig_route_check.py. In the mixed device calls a family's packed rows are
// dense, but only the device knows how many there are; the host sizes every launch and
// every buffer for a bound. The three passes are replayed here wave by wave -- the
// count clipped to the bound (route_count_clip, rsa_route_launch_count), the match, a
// wave's ballots, one reservation per list and wave, the ranked writes -- into heap
// buffers of exactly the sizes the layouts name for the bound (key rows, route ids,
// lists, perm), and compared with a plain sequential partition of rows 0 .. count
// that knows nothing of waves:
//   no row at or past the count is in any list or class, and its route id is not written;
//   nothing is written past a list's count (the fill pattern survives);
//   the counts, the lists (sorted) and the cumulative totals are the sequential ones;
//   ECDSA: perm holds the seven classes' runs in order, the generic five first, each
//     what the unrouted partition holds for those lanes;
//   RSA: the launch loop over workspaces of 64 and 4,096 rows clips each launch's rows,
//     a launch wholly past the count lists nothing, rows the prep decided are in neither
//     list but in the totals.
// Counts relative to the bound: 0, 1, 63, 64, 65, bound - 1, bound, bound + 5 and 2^32 - 1
// (both clipped). Bounds: the tile edges (Ed25519 2,048 / 2,049, ECDSA 4,096 / 4,097,
// RSA 256 / 257) and 100. Waves in order and shuffled.
// Usage: sig_route_check <seed>; prints one JSON line, exit 0 = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../corda_amd/csrc/ecdsa_route.hpp"
#include "../corda_amd/csrc/ed25519_route.hpp"
#include "../corda_amd/csrc/rsa_route.hpp"

using namespace cordahip;

static uint64_t rng_state;
static uint64_t rng() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

static uint64_t failures = 0, ed_cases = 0, ec_cases = 0, rsa_cases = 0, clipped_cases = 0, rows_routed = 0,
                rows_past = 0, keyed_seen = 0, empty_launches = 0, decided_seen = 0;
#define CHECK(c)                                                           \
  do {                                                                     \
    if (!(c)) {                                                            \
      if (failures++ < 20) fprintf(stderr, "line %d: %s\n", __LINE__, #c); \
    }                                                                      \
  } while (0)

constexpr uint32_t kFill = 0xA5A5A5A5u;

// the order in which the waves of `blocks` blocks of 256 threads reserve their ranges
static std::vector<uint64_t> wave_order(uint64_t blocks, bool shuffle) {
  std::vector<uint64_t> order(blocks * 4);
  std::iota(order.begin(), order.end(), 0);
  if (shuffle)
    for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[rng() % i]);
  return order;
}

// the counts to try against a bound
static std::vector<uint32_t> counts_for(uint64_t bound) {
  std::vector<uint32_t> c = {0u, 1u, 63u, 64u, 65u, (uint32_t)(bound - 1), (uint32_t)bound, (uint32_t)(bound + 5),
                             0xFFFFFFFFu};
  return c;
}

// ---------------------------------------------------------------------------
// Ed25519 (ed25519_route_kernel with count)

struct EdTable {
  std::vector<uint32_t> recs = std::vector<uint32_t>(kVkeySlots * kVkeyRecWords, 0u);
  void put(uint32_t slot, const uint32_t a[8], uint32_t gen) {
    uint32_t* r = &recs[slot * kVkeyRecWords];
    r[kVkeyRecLive] = 1;
    r[kVkeyRecId] = vkey_make_id(slot, gen);
    memcpy(r + kVkeyRecAbyte, a, 32);
  }
};

// keyed[i]: row i carries the registered key K (every row of the bound has key bytes: rows
// past the count hold whatever an earlier batch left, here registered keys on purpose)
static void ed_case(const EdTable& t, const uint32_t K[8], uint64_t n, uint32_t count, const std::vector<uint8_t>& is_k,
                    bool shuffle) {
  ed_cases++;
  const uint64_t m = route_count_clip(count, n);
  CHECK(m <= n && (count > n ? m == n : m == count));
  if (count > n) clipped_cases++;
  uint32_t* keys = new uint32_t[n * 8];  // exactly the bound's rows
  for (uint64_t i = 0; i < n; i++)
    for (int q = 0; q < 8; q++) keys[i * 8 + q] = is_k[i] ? K[q] : (uint32_t)rng() | 1u;
  uint32_t* gathered = new uint32_t[kVkeySlots * kRouteRecWords];  // the block's LDS
  const uint32_t nlive = route_gather(gathered, t.recs.data());
  const uint64_t words = route_scratch_words(n);  // the layout of the bound, exactly
  uint32_t* scratch = new uint32_t[words];
  memset(scratch, 0xA5, words * 4);
  scratch[kRouteCntKeyed] = scratch[kRouteCntGeneric] = 0;  // the launcher's memset
  uint32_t* route = scratch + route_off_route(n);
  uint32_t* keyed = scratch + route_off_keyed(n);
  uint32_t* generic = scratch + route_off_generic(n);
  uint64_t totals[2] = {0, 0};
  const uint64_t blocks = (n + kRouteTile - 1) / kRouteTile;  // the grid follows the bound
  for (uint64_t w : wave_order(blocks, shuffle)) {
    const uint64_t tile = w / 4;
    const uint32_t wave = (uint32_t)(w % 4);
    uint64_t bk[kRouteIter], bg[kRouteIter];
    uint32_t nk = 0, ng = 0;
    for (int it = 0; it < kRouteIter; it++) {
      bk[it] = bg[it] = 0;
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t i = route_tile_lane(tile, it, wave * 64 + lane);
        if (i >= m) continue;
        const uint32_t id = route_match(keys + i * 8, gathered, nlive);
        route[i] = id;
        (id != kVkeyNoId ? bk[it] : bg[it]) |= 1ull << lane;
      }
      nk += (uint32_t)__builtin_popcountll(bk[it]);
      ng += (uint32_t)__builtin_popcountll(bg[it]);
    }
    uint32_t sk = 0, sg = 0;
    if (nk) {
      sk = scratch[kRouteCntKeyed];
      scratch[kRouteCntKeyed] += nk;
      totals[0] += nk;
    }
    if (ng) {
      sg = scratch[kRouteCntGeneric];
      scratch[kRouteCntGeneric] += ng;
      totals[1] += ng;
    }
    for (int it = 0; it < kRouteIter; it++) {
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t i = (uint32_t)route_tile_lane(tile, it, wave * 64 + lane);
        if ((bk[it] >> lane) & 1) keyed[sk + route_rank(bk[it], lane)] = i;
        if ((bg[it] >> lane) & 1) generic[sg + route_rank(bg[it], lane)] = i;
      }
      sk += (uint32_t)__builtin_popcountll(bk[it]);
      sg += (uint32_t)__builtin_popcountll(bg[it]);
    }
  }
  // the sequential partition of rows 0 .. count
  std::vector<uint32_t> want_k, want_g;
  for (uint64_t i = 0; i < m; i++) (is_k[i] && nlive ? want_k : want_g).push_back((uint32_t)i);
  rows_routed += m;
  rows_past += n - m;
  keyed_seen += want_k.size();
  const uint32_t ck = scratch[kRouteCntKeyed], cg = scratch[kRouteCntGeneric];
  CHECK(ck == want_k.size() && cg == want_g.size() && (uint64_t)ck + cg == m);
  CHECK(totals[0] == want_k.size() && totals[1] == want_g.size());
  if (ck == want_k.size() && cg == want_g.size()) {
    std::vector<uint32_t> gk(keyed, keyed + ck), gg(generic, generic + cg);
    std::sort(gk.begin(), gk.end());
    std::sort(gg.begin(), gg.end());
    CHECK(gk == want_k && gg == want_g);  // hence no row at or past the count in a list
  }
  // nothing past a list's count, no route id at or past the count, the header's spare words
  for (uint64_t j = ck; j < n; j++) CHECK(keyed[j] == kFill);
  for (uint64_t j = cg; j < n; j++) CHECK(generic[j] == kFill);
  for (uint64_t i = m; i < n; i++) CHECK(route[i] == kFill);
  for (uint64_t i = 0; i < m; i++) CHECK((route[i] != kVkeyNoId) == (is_k[i] && nlive != 0));
  for (uint32_t j = 2; j < kRouteHdrWords; j++) CHECK(scratch[j] == kFill);
  delete[] scratch;
  delete[] gathered;
  delete[] keys;
}

// ---------------------------------------------------------------------------
// ECDSA (ecdsa_route_kernel and ecdsa_scatter_routed_kernel with count)

struct Point {
  uint32_t x[8], y[8];
};
struct EcTable {
  std::vector<uint32_t> recs = std::vector<uint32_t>(kVkeySlots * kEcVkeyRecWords, 0u);
  std::vector<uint32_t> points = std::vector<uint32_t>(kVkeySlots * 16, 0u);
  void put(uint32_t slot, uint32_t scheme, const Point& p, uint32_t gen) {
    uint32_t* r = &recs[slot * kEcVkeyRecWords];
    r[kEcVkeyRecScheme] = scheme;
    r[kEcVkeyRecId] = vkey_make_id(slot, gen);
    r[kEcVkeyRecLive] = 1;
    memcpy(&points[slot * 16], p.x, 32);
    memcpy(&points[slot * 16 + 8], p.y, 32);
  }
};
struct Lane {
  uint8_t scheme, key_len, keyed;  // keyed: the bytes encode a registered point of the scheme
  uint8_t key[65];
};
static void be32(uint8_t out[32], const uint32_t w[8]) {
  for (int b = 0; b < 32; b++) out[b] = (uint8_t)(w[7 - b / 4] >> (8 * (3 - b % 4)));
}
static Lane ec_lane(uint8_t scheme, const Point& p, bool compressed, bool keyed) {
  Lane l;
  l.scheme = scheme;
  l.key_len = compressed ? 33 : 65;
  l.keyed = keyed;
  be32(l.key + 1, p.x);
  be32(l.key + 33, p.y);
  l.key[0] = compressed ? (uint8_t)(2 | (p.y[0] & 1)) : 4;
  return l;
}
static int ref_class(const Lane& l, bool keyed) {
  if (keyed) return l.scheme == 2 ? 5 : 6;
  if (l.scheme == 2) return l.key_len == 33 ? 1 : 0;
  if (l.scheme == 3) return l.key_len == 33 ? 3 : 2;
  return 4;
}

static void ec_case(const EcTable& t, const std::vector<Lane>& lanes, uint32_t count, bool shuffle) {
  ec_cases++;
  const uint64_t n = lanes.size();
  uint64_t m = route_count_clip(count, n);  // each kernel clips what it reads
  if (count > n) clipped_cases++;
  uint8_t* scheme = new uint8_t[n];
  uint8_t* key_len = new uint8_t[n];
  uint8_t* keys = new uint8_t[n * 65];
  for (uint64_t i = 0; i < n; i++) {
    scheme[i] = lanes[i].scheme;
    key_len[i] = lanes[i].key_len;
    memcpy(keys + i * 65, lanes[i].key, 65);
  }
  const uint64_t words = ec_route_scratch_words(n);
  uint32_t* scratch = new uint32_t[words];
  memset(scratch, 0xA5, words * 4);
  uint32_t* perm = new uint32_t[n];  // the slot's perm, exactly the bound's words
  memset(perm, 0xA5, n * 4);
  uint32_t counters[2 * kEcRouteClasses] = {};  // the launcher's memset
  uint32_t* counts = counters;
  uint32_t* cursors = counters + kEcRouteClasses;
  uint64_t totals[2] = {0, 0};
  uint32_t* route = scratch + ec_route_off_route();
  const uint32_t nlive = ec_route_gather(scratch + kEcRouteRecBase, t.recs.data(), t.points.data());
  scratch[kEcRouteCntLive] = nlive;
  const uint32_t* gathered = scratch + kEcRouteRecBase;
  const uint64_t blocks = (n + kEcRouteTile - 1) / kEcRouteTile;  // the grid follows the bound

  // route: a block's class totals, one add per class
  for (uint64_t block = 0; block < blocks; block++) {
    uint32_t tot[kEcRouteClasses] = {};
    for (uint32_t th = 0; th < 256; th++)
      for (int it = 0; it < kEcRouteIter; it++) {
        const uint64_t i = ec_route_tile_lane(block, it, th);
        if (i >= m) continue;
        const uint32_t id = ec_route_match(scheme[i], key_len[i], keys + i * 65, gathered, nlive);
        route[i] = id;
        tot[ec_route_class(scheme[i], key_len[i], id)]++;
      }
    for (int k = 0; k < kEcRouteClasses; k++) {
      counts[k] += tot[k];
      totals[k < kEcRouteGenericClasses ? 1 : 0] += tot[k];
    }
  }
  // scatter: the count read again, a wave's ballots, one reservation per class, ranked writes
  m = route_count_clip(count, n);
  for (uint64_t w : wave_order(blocks, shuffle)) {
    const uint64_t block = w / 4;
    const uint32_t wave = (uint32_t)(w % 4);
    uint64_t bal[kEcRouteIter][kEcRouteClasses];
    uint32_t tot[kEcRouteClasses] = {};
    for (int it = 0; it < kEcRouteIter; it++) {
      for (int k = 0; k < kEcRouteClasses; k++) bal[it][k] = 0;
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t i = ec_route_tile_lane(block, it, wave * 64 + lane);
        if (i < m) bal[it][ec_route_class(scheme[i], key_len[i], route[i])] |= 1ull << lane;
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
    }
    for (int it = 0; it < kEcRouteIter; it++)
      for (int k = 0; k < kEcRouteClasses; k++) {
        for (uint32_t lane = 0; lane < 64; lane++)
          if ((bal[it][k] >> lane) & 1)
            perm[start[k] + route_rank(bal[it][k], lane)] = (uint32_t)ec_route_tile_lane(block, it, wave * 64 + lane);
        start[k] += (uint32_t)__builtin_popcountll(bal[it][k]);
      }
  }
  // the sequential partition of rows 0 .. count
  std::vector<uint32_t> want[kEcRouteClasses];
  for (uint64_t i = 0; i < m; i++) {
    const bool k = lanes[i].keyed && nlive;
    want[ref_class(lanes[i], k)].push_back((uint32_t)i);
    keyed_seen += k;
    CHECK((route[i] != kVkeyNoId) == k);
  }
  rows_routed += m;
  rows_past += n - m;
  uint64_t at = 0, tk = 0, tg = 0;
  bool counts_ok = true;
  for (int k = 0; k < kEcRouteClasses; k++) {
    counts_ok = counts_ok && counts[k] == want[k].size() && cursors[k] == counts[k];
    (k < kEcRouteGenericClasses ? tg : tk) += want[k].size();
  }
  CHECK(counts_ok);
  CHECK(totals[0] == tk && totals[1] == tg && tk + tg == m);
  CHECK(ec_route_generic_count(counts) == tg && ec_route_keyed_start(counts, 2) == tg &&
        ec_route_keyed_start(counts, 3) == tg + counts[5]);
  if (counts_ok) {
    for (int k = 0; k < kEcRouteClasses; k++) {
      std::vector<uint32_t> got(perm + at, perm + at + counts[k]);
      std::sort(got.begin(), got.end());
      CHECK(got == want[k]);  // the generic five: what the unrouted partition holds for those lanes
      at += counts[k];
    }
    CHECK(at == m);
  }
  for (uint64_t j = m; j < n; j++) CHECK(perm[j] == kFill);  // nothing past the lists
  for (uint64_t i = m; i < n; i++) CHECK(route[i] == kFill);
  for (uint32_t j = 1; j < kEcRouteRecBase; j++) CHECK(scratch[j] == kFill);
  delete[] perm;
  delete[] scratch;
  delete[] keys;
  delete[] key_len;
  delete[] scheme;
}

// ---------------------------------------------------------------------------
// RSA (rsa_launch_count_kernel's clip and rsa_route_kernel with the launch's count)

constexpr uint32_t kW = 64;
constexpr uint8_t kOkStatus = 0, kDecided = 3;
struct RsaRow {
  uint8_t keyed, st;
};

static void rsa_case(const std::vector<uint32_t>& tab, const uint32_t* K, uint32_t Ke, const std::vector<RsaRow>& rows,
                     uint32_t count, uint64_t ws_rows, bool shuffle) {
  rsa_cases++;
  const uint64_t n = rows.size();  // the class's bound (sigpack rsa_cap_rows)
  if (count > n) clipped_cases++;
  const uint64_t mcount = route_count_clip(count, n);
  uint32_t* cand = new uint32_t[(size_t)kVkeySlots * kRsaRouteCandWords];
  const uint32_t ncand = rsa_route_gather(cand, tab.data());
  const uint64_t cap = std::min<uint64_t>(ws_rows, (n + 63) / 64 * 64);  // runtime.cpp: the largest launch
  const uint64_t words = rsa_route_scratch_words(cap);
  uint32_t* scratch = new uint32_t[words];
  memset(scratch, 0xA5, words * 4);
  uint32_t* route = scratch + rsa_route_off_route(cap);
  uint32_t* keyed = scratch + rsa_route_off_keyed(cap);
  uint32_t* generic = scratch + rsa_route_off_generic(cap);
  uint64_t totals[2] = {0, 0}, want_tk = 0, want_tg = 0, listed_rows = 0;
  for (uint64_t lo = 0; lo < n; lo += ws_rows) {
    const uint64_t m = rsa_route_launch_rows(ws_rows, n, lo);
    // the head's one-thread kernel, then the route pass's own clip of what it reads
    const uint32_t lc = (uint32_t)rsa_route_launch_count(count, lo, m);
    const uint64_t mm = route_count_clip(lc, m);
    CHECK(mm <= m && mm == (mcount > lo ? std::min<uint64_t>(mcount - lo, m) : 0));
    if (!mm) empty_launches++;
    uint32_t* mod = new uint32_t[m * kW];  // the launch's rows of the bound, exactly
    uint32_t* exp = new uint32_t[m];
    uint8_t* st = new uint8_t[mm ? mm : 1];  // the prep stops at the count: no status behind it
    for (uint64_t i = 0; i < m; i++) {
      for (uint32_t q = 0; q < kW; q++) mod[i * kW + q] = rows[lo + i].keyed ? K[q] : (uint32_t)rng() | 1u;
      exp[i] = rows[lo + i].keyed ? Ke : 65537u;
      if (i < mm) st[i] = rows[lo + i].st;
    }
    memset(scratch + kRsaRouteHdrWords, 0xA5, (words - kRsaRouteHdrWords) * 4);
    scratch[kRsaRouteCntKeyed] = scratch[kRsaRouteCntGeneric] = 0;  // the launcher's memset
    const uint64_t blocks = (m + kRsaRouteBlock - 1) / kRsaRouteBlock;  // the grid follows the bound
    for (uint64_t w : wave_order(blocks, shuffle)) {
      const uint64_t block = w / 4;
      const uint32_t wave = (uint32_t)(w % 4);
      uint64_t mk = 0, mg = 0, lk = 0, lg = 0;
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t i = rsa_route_row(block, wave * 64 + lane);
        if (i >= mm) continue;
        const uint32_t id = rsa_route_match(kW, exp[i], mod + i * kW, cand, ncand, tab.data());
        route[i] = id;
        const bool k = id != kVkeyNoId, listed = st[i] == kOkStatus;
        (k ? mk : mg) |= 1ull << lane;
        if (listed) (k ? lk : lg) |= 1ull << lane;
      }
      uint32_t sk = 0, sg = 0;
      if (lk) {
        sk = scratch[kRsaRouteCntKeyed];
        scratch[kRsaRouteCntKeyed] += (uint32_t)__builtin_popcountll(lk);
      }
      if (lg) {
        sg = scratch[kRsaRouteCntGeneric];
        scratch[kRsaRouteCntGeneric] += (uint32_t)__builtin_popcountll(lg);
      }
      totals[0] += (uint64_t)__builtin_popcountll(mk);
      totals[1] += (uint64_t)__builtin_popcountll(mg);
      for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t i = (uint32_t)rsa_route_row(block, wave * 64 + lane);
        if ((lk >> lane) & 1) keyed[sk + route_rank(lk, lane)] = i;
        if ((lg >> lane) & 1) generic[sg + route_rank(lg, lane)] = i;
      }
    }
    std::vector<uint32_t> want_k, want_g;
    for (uint64_t i = 0; i < mm; i++) {
      const bool k = rows[lo + i].keyed && ncand;
      (k ? want_tk : want_tg)++;
      keyed_seen += k;
      CHECK((route[i] != kVkeyNoId) == k);
      if (rows[lo + i].st != kOkStatus) {
        decided_seen++;
        continue;
      }
      (k ? want_k : want_g).push_back((uint32_t)i);
    }
    rows_routed += mm;
    rows_past += m - mm;
    const uint32_t ck = scratch[kRsaRouteCntKeyed], cg = scratch[kRsaRouteCntGeneric];
    CHECK(ck == want_k.size() && cg == want_g.size());
    if (ck == want_k.size() && cg == want_g.size()) {
      std::vector<uint32_t> gk(keyed, keyed + ck), gg(generic, generic + cg);
      std::sort(gk.begin(), gk.end());
      std::sort(gg.begin(), gg.end());
      CHECK(gk == want_k && gg == want_g);
      listed_rows += ck + cg;
    }
    for (uint64_t j = ck; j < cap; j++) CHECK(keyed[j] == kFill);
    for (uint64_t j = cg; j < cap; j++) CHECK(generic[j] == kFill);
    for (uint64_t i = mm; i < cap; i++) CHECK(route[i] == kFill);
    for (uint32_t j = 2; j < kRsaRouteHdrWords; j++) CHECK(scratch[j] == kFill);
    delete[] st;
    delete[] exp;
    delete[] mod;
  }
  CHECK(totals[0] == want_tk && totals[1] == want_tg && totals[0] + totals[1] == mcount);
  CHECK(listed_rows <= mcount);
  delete[] scratch;
  delete[] cand;
}

int main(int argc, char** argv) {
  rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  CHECK(route_count_clip(0, 5) == 0 && route_count_clip(5, 5) == 5 && route_count_clip(6, 5) == 5 &&
        route_count_clip(0xFFFFFFFFull, 1) == 1);
  CHECK(rsa_route_launch_count(130, 0, 64) == 64 && rsa_route_launch_count(130, 128, 64) == 2 &&
        rsa_route_launch_count(128, 128, 64) == 0 && rsa_route_launch_count(0xFFFFFFFFull, 64, 64) == 64 &&
        rsa_route_launch_count(3, 64, 64) == 0);

  // row patterns: every row keyed, none, one keyed row in a wave, random halves
  const auto pattern = [](int pat, uint64_t i) {
    switch (pat) {
      case 0: return true;
      case 1: return false;
      case 2: return i % 64 == 37;
      default: return rng() % 2 == 0;
    }
  };

  {  // Ed25519
    uint32_t K[8];
    for (int q = 0; q < 8; q++) K[q] = (uint32_t)rng();
    EdTable none, one;
    one.put(17, K, 3);
    for (const EdTable* t : {&none, &one})
      for (uint64_t n : {(uint64_t)kRouteTile, (uint64_t)kRouteTile + 1, (uint64_t)100})
        for (uint32_t count : counts_for(n))
          for (int pat = 0; pat < 4; pat++) {
            std::vector<uint8_t> is_k(n);
            for (uint64_t i = 0; i < n; i++) is_k[i] = pattern(pat, i);
            ed_case(*t, K, n, count, is_k, false);
            ed_case(*t, K, n, count, is_k, true);
          }
  }
  {  // ECDSA: a live key on each curve; lanes on both curves, compressed and not, and class "other"
    Point P2, P3;
    for (int q = 0; q < 8; q++) {
      P2.x[q] = (uint32_t)rng(), P2.y[q] = (uint32_t)rng();
      P3.x[q] = (uint32_t)rng(), P3.y[q] = (uint32_t)rng();
    }
    EcTable none, two;
    two.put(5, 2, P2, 1);
    two.put(40, 3, P3, 2);
    for (const EcTable* t : {&none, &two})
      for (uint64_t n : {(uint64_t)kEcRouteTile, (uint64_t)kEcRouteTile + 1, (uint64_t)100})
        for (uint32_t count : counts_for(n))
          for (int pat = 0; pat < 4; pat++) {
            std::vector<Lane> lanes(n);
            for (uint64_t i = 0; i < n; i++) {
              const bool k = pattern(pat, i);
              const uint8_t scheme = (uint8_t)(2 + rng() % 2);
              const bool comp = rng() % 2;
              if (k) {
                lanes[i] = ec_lane(scheme, scheme == 2 ? P2 : P3, comp, true);
              } else {
                Point q;
                for (int z = 0; z < 8; z++) q.x[z] = (uint32_t)rng(), q.y[z] = (uint32_t)rng();
                lanes[i] = ec_lane(scheme, q, comp, false);
                if (pat == 3 && rng() % 8 == 0) lanes[i].scheme = 1;  // class "other"
                // the other curve's registered point: a miss
                if (pat == 3 && rng() % 8 == 0) lanes[i] = ec_lane(scheme, scheme == 2 ? P3 : P2, comp, false);
              }
            }
            ec_case(*t, lanes, count, false);
            ec_case(*t, lanes, count, true);
          }
  }
  {  // RSA-2048 rows, one live key; workspaces of 64 rows (the launch loop) and 4,096
    std::vector<uint32_t> none((size_t)kVkeySlots * rsa::kVkeyRecWords, 0u), one = none;
    uint32_t K[kW];
    for (uint32_t q = 0; q < kW; q++) K[q] = (uint32_t)rng();
    K[0] |= 1u;
    {
      uint32_t* r = &one[(size_t)9 * rsa::kVkeyRecWords];
      r[rsa::kVkeyRecIdWord] = vkey_make_id(9, 4);
      r[rsa::kVkeyRecEWord] = 65537u;
      r[rsa::kVkeyRecWordsWord] = kW;
      memcpy(r + rsa::kVkeyRecNWord, K, sizeof K);
    }
    for (const std::vector<uint32_t>* t : {&none, &one})
      for (uint64_t n : {(uint64_t)kRsaRouteBlock, (uint64_t)kRsaRouteBlock + 1, (uint64_t)100})
        for (uint32_t count : counts_for(n))
          for (int pat = 0; pat < 4; pat++) {
            std::vector<RsaRow> rows(n);
            for (uint64_t i = 0; i < n; i++) {
              rows[i].keyed = pattern(pat, i);
              rows[i].st = pat == 3 && i % 5 == 3 ? kDecided : kOkStatus;
            }
            for (uint64_t ws : {(uint64_t)64, (uint64_t)4096}) {
              rsa_case(*t, K, 65537u, rows, count, ws, false);
              rsa_case(*t, K, 65537u, rows, count, ws, true);
            }
          }
  }
  printf("{\"ok\": %s, \"failures\": %llu, \"ed_cases\": %llu, \"ec_cases\": %llu, \"rsa_cases\": %llu, "
         "\"clipped_cases\": %llu, \"rows_routed\": %llu, \"rows_past\": %llu, \"keyed\": %llu, "
         "\"empty_launches\": %llu, \"decided\": %llu}\n",
         failures ? "false" : "true", (unsigned long long)failures, (unsigned long long)ed_cases,
         (unsigned long long)ec_cases, (unsigned long long)rsa_cases, (unsigned long long)clipped_cases,
         (unsigned long long)rows_routed, (unsigned long long)rows_past, (unsigned long long)keyed_seen,
         (unsigned long long)empty_launches, (unsigned long long)decided_seen);
  return failures ? 1 : 0;
}
