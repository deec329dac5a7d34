// Mutation fuzzer of the FilteredTransaction build (cordahip_filtered_tx_build):
// its batch validation (corda_amd/csrc/csr_check.hpp check_filtered_build_batch)
// and the core K10 runs per transaction (corda_amd/csrc/pmt_core.hpp), compiled
// for the host, built by tests/test_pmt_build_fuzz.py with
// g++ -fsanitize=address,undefined. The node hash is a cheap stand-in mixing
// function (the core takes it as a template parameter; SHA-256 itself is tested
// on the GPU), the Z_j table is derived from it as kZeroHash is from SHA-256.
//
// Every array lives in a heap block of exactly its declared size -- offsets
// [n + 1], include [nleaves], the workspace 2 * nleaves hashes and 3 * nleaves
// bytes, tok [ntok], tok_hash [32 * ntok], txid [32 * ntx], counts and statuses
// [ntx] -- so an access past one is an ASan report.
//
// Part one: per round a batch is built valid -- transaction sizes from 0, 1,
// powers of two and their neighbours, leaf hashes with duplicates inside a
// transaction, masks none / all / one / random, slots of the bound or a little
// more -- then (most rounds) mutated: an offset of any level, a declared count,
// or one transaction's slot shortened. check_filtered_build_batch must reject
// exactly what the contract rejects.
// Part two: whenever the leaf level is sound (what the device-resident call
// takes on trust), every lane runs the core exactly as the kernel does
// (build_lane: the slot judged from the offsets as they are) and its id,
// status, count and tokens are compared with an independent recursive build
// over the explicitly padded tree; a lane that reports a failure must leave its
// slot untouched, and no lane may write outside its slot.
// Exit 0 when everything matches; a sanitizer report aborts the process.
//
// usage: pmt_build_fuzz ROUNDS RNG_SEED   (prints one JSON line of counts)
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

#include "../corda_amd/csrc/csr_check.hpp"
#include "../corda_amd/csrc/pmt_core.hpp"

using namespace cordahip;
using namespace cordahip::rt;

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
  uint64_t n = 0;
  void make(uint64_t k, int fill = 0) {
    n = k;
    p.reset(new T[k ? k : 1]);
    if (k) std::memset(p.get(), fill, sizeof(T) * k);
  }
  T* get() const { return n ? p.get() : nullptr; }
};

struct SerialPar {
  template <class F>
  void operator()(uint64_t n, uint64_t, F&& fn) const {
    if (n) fn(0, n);
  }
};

void mutate_off(Rng& r, Arr<uint64_t>& off, uint64_t limit) {
  if (off.n == 0) return;
  const uint64_t i = r.below(off.n);
  uint64_t& v = off.p[i];
  switch (r.below(7)) {
    case 0: v = 0; break;
    case 1: v += 1 + r.below(5); break;
    case 2: v = v > 5 ? v - 1 - r.below(5) : 0; break;
    case 3: v = limit + r.below(2); break;
    case 4: v = UINT64_MAX - r.below(3); break;
    case 5: v = r.next(); break;
    default:
      if (i + 1 < off.n) std::swap(off.p[i], off.p[i + 1]);
      break;
  }
}

// contract: off[a..b] non-decreasing and off[b] <= limit (ground truth, no shortcuts)
bool truth(const Arr<uint64_t>& off, uint64_t a, uint64_t b, uint64_t limit) {
  if (b < a || b >= off.n) return false;
  for (uint64_t i = a; i < b; i++)
    if (off.p[i] > off.p[i + 1]) return false;
  return off.p[b] <= limit;
}

// ---- the stand-in node hash and its padding constants -------------------------
typedef std::array<uint32_t, 8> Hash;
inline uint32_t rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }
void mix(uint32_t out[8], const uint32_t a[8], const uint32_t b[8]) {  // order-sensitive, cheap
  uint32_t t[8];
  for (int k = 0; k < 8; k++)
    t[k] = rotl(a[k] * 0x9e3779b1u + 0x7f4a7c15u, 5 + k) ^ (b[(k + 3) & 7] * 0x85ebca6bu + (uint32_t)k);
  for (int k = 0; k < 8; k++) out[k] = t[k] + rotl(t[(k + 1) & 7], 13) + 0xc2b2ae35u;
}
Hash g_zero[64];
struct Mix {
  void operator()(uint32_t out[8], const uint32_t a[8], const uint32_t b[8]) const { mix(out, a, b); }
};
struct Zero {
  void operator()(int level, uint32_t out[8]) const {
    for (int k = 0; k < 8; k++) out[k] = g_zero[level][k];
  }
};

// ---- the independent build: MerkleTree.getMerkleTree + PartialMerkleTree.build,
// recursively over the explicitly padded leaf list (every padding node hashed) ----
struct Tok {
  uint8_t kind;
  Hash h;
};
struct Model {
  std::vector<Hash> leaves;  // padded to a power of two with zero hashes
  uint64_t m = 0;
  std::set<Hash> include;    // includeHashes as a set (membership by hash)
  uint64_t used = 0;
  std::vector<Tok> toks;
  // returns (hash of the subtree, an included leaf lies below); emits its partial tree
  std::pair<Hash, bool> rec(uint64_t lo, uint64_t n) {
    if (n == 1) {
      const bool in = lo < m && include.count(leaves[lo]) != 0;
      used += in;
      toks.push_back({in ? pmt::kTokIncluded : pmt::kTokLeaf, leaves[lo]});
      return {leaves[lo], in};
    }
    const size_t mark = toks.size();
    const auto l = rec(lo, n / 2), r = rec(lo + n / 2, n / 2);
    Hash h;
    mix(h.data(), l.first.data(), r.first.data());
    if (l.second || r.second) {
      toks.push_back({pmt::kTokNode, Hash{}});
      return {h, true};
    }
    toks.resize(mark);
    toks.push_back({pmt::kTokLeaf, h});
    return {h, false};
  }
};

struct Stats {
  uint64_t batches = 0, invalid = 0, lanes = 0, tokens = 0, status[16] = {};
};

const uint64_t kSizes[] = {0, 1, 1, 2, 3, 4, 5, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33};

bool round(Rng& r, Stats& st) {
  const uint64_t ntx = r.below(20);
  Arr<uint64_t> tlo, lo, tko;
  tlo.make(ntx + 1);
  tko.make(ntx + 1);
  uint64_t nleaves = 0, ntok = r.below(3);  // the first slot need not start at 0
  std::vector<uint64_t> ms(ntx);
  for (uint64_t t = 0; t < ntx; t++) {
    const uint64_t m = r.chance(80) ? kSizes[r.below(sizeof(kSizes) / sizeof(kSizes[0]))] : r.below(41);
    ms[t] = m;
    tlo.p[t] = nleaves;
    tko.p[t] = ntok;
    nleaves += m;
    uint64_t need;
    if (!pmt::slot_bound(m, &need)) return false;
    ntok += need + (r.chance(25) ? r.below(4) : 0);
  }
  if (ntx) tlo.p[ntx] = nleaves, tko.p[ntx] = ntok;
  ntok += r.below(3);  // and the last need not end at ntok
  lo.make(nleaves + 1);
  uint64_t lb = 0;
  for (uint64_t i = 0; i < nleaves; i++) lo.p[i] = lb, lb += r.below(20);
  lo.p[nleaves] = lb;
  // leaf hashes (nonzero words: a zero hash has no preimage), duplicates inside a transaction, masks
  Arr<uint32_t> hashes;
  Arr<uint8_t> include;
  hashes.make(nleaves * 8);
  include.make(nleaves);
  for (uint64_t t = 0; t < ntx; t++) {
    const uint64_t l0 = tlo.p[t], m = ms[t];
    const uint64_t dup = r.below(4);  // 0: none, 1: a few, 2: many, 3: all equal
    for (uint64_t i = 0; i < m; i++) {
      const bool copy = i && (dup == 3 || (dup == 2 && r.chance(50)) || (dup == 1 && r.chance(10)));
      const uint64_t src = copy ? r.below(i) : i;
      for (int k = 0; k < 8; k++)
        hashes.p[(l0 + i) * 8 + k] = copy ? hashes.p[(l0 + src) * 8 + k] : (uint32_t)r.next() | 1u;
    }
    const uint64_t mode = r.below(5);  // none, all, one, sparse, dense
    for (uint64_t i = 0; i < m; i++)
      include.p[l0 + i] = mode == 1   ? 1
                          : mode == 3 ? r.chance(15)
                          : mode == 4 ? (uint8_t)(r.chance(70) * 0x80)  // any nonzero byte selects
                                      : 0;
    if (mode == 2 && m) include.p[l0 + r.below(m)] = 7;
  }
  // ---- part one: mutate, validate ----
  uint64_t nl = nleaves, nt = ntok, lbl = lb;
  if (r.chance(70)) {
    switch (r.below(8)) {
      case 0: mutate_off(r, tlo, nleaves); break;
      case 1: mutate_off(r, lo, lb); break;
      case 2: mutate_off(r, tko, ntok); break;
      case 3: nl = nl ? nl - 1 : 0; break;
      case 4: nt = nt ? nt - 1 - r.below(std::min<uint64_t>(nt, 3)) : 0; break;
      case 5: lbl = lbl ? lbl - 1 : 0; break;
      default:  // one transaction's slot shortened: the later offsets move down
        if (ntx) {
          const uint64_t t = r.below(ntx), cut = 1 + r.below(2);
          for (uint64_t i = t + 1; i <= ntx; i++) tko.p[i] = tko.p[i] >= cut ? tko.p[i] - cut : 0;
        }
        break;
    }
  }
  const bool leaf_level = ntx == 0 || truth(tlo, 0, ntx, nl);
  bool valid = true;
  if (ntx) {
    valid = leaf_level && truth(lo, tlo.p[0], tlo.p[ntx], lbl) && truth(tko, 0, ntx, nt);
    for (uint64_t t = 0; valid && t < ntx; t++) {
      const uint64_t m = tlo.p[t + 1] - tlo.p[t];
      uint64_t p = 1;
      while (p < m) p *= 2;
      if (tko.p[t + 1] - tko.p[t] < (m ? 2 * p - 1 : 0)) valid = false;
    }
  }
  Arr<uint64_t> lo_d;
  lo_d.make(std::min<uint64_t>(lo.n, nl + 1));
  if (lo_d.n) std::memcpy(lo_d.p.get(), lo.p.get(), lo_d.n * 8);
  Arr<uint8_t> leaf_bytes, tok, tok_hash, txid, txst;
  Arr<uint64_t> cnt;
  leaf_bytes.make(lbl);
  tok.make(nt, 0xEE);
  tok_hash.make(nt * 32, 0xEE);
  txid.make(ntx * 32, 0xEE);
  txst.make(ntx, 0xEE);
  cnt.make(ntx, 0xEE);
  cordahip_filtered_build_batch b{ntx, leaf_bytes.get(), lo_d.get(), tlo.get(), include.get(), tko.get(), txid.get(),
                                  tok.get(), tok_hash.get(), cnt.get(), txst.get(), nl, lbl, nt};
  const bool ok = check_filtered_build_batch(SerialPar{}, &b);
  st.batches++;
  st.invalid += !ok;
  if (ok != valid) {
    fprintf(stderr, "build batch: check says %s, the contract %s\n", ok ? "valid" : "invalid",
            valid ? "valid" : "invalid");
    return false;
  }
  // ---- part two: the core, lane by lane, against the recursive build ----
  // (the leaf level sound and within the arrays that exist: the device call's contract)
  if (!ntx || !leaf_level || tlo.p[ntx] > nleaves) return true;
  Arr<uint32_t> up;
  Arr<uint8_t> has;
  up.make(nleaves * 16, 0xEE);
  has.make(nleaves * 3, 0xEE);
  std::vector<uint8_t> tok_before(nt), hash_before(nt * 32);
  for (uint64_t t = 0; t < ntx; t++) {
    if (nt) std::memcpy(tok_before.data(), tok.p.get(), nt), std::memcpy(hash_before.data(), tok_hash.p.get(), nt * 32);
    pmt::build_lane(t, hashes.get(), tlo.get(), include.get(), tko.get(), nt, up.get(), has.get(), txid.get(),
                    tok.get(), tok_hash.get(), cnt.get(), txst.get(), Mix{}, Zero{});
    st.lanes++;
    const uint64_t l0 = tlo.p[t], m = tlo.p[t + 1] - l0;
    const uint64_t k0 = tko.p[t], k1 = tko.p[t + 1];
    const bool slot = k0 <= k1 && k1 <= nt;
    const uint64_t cap = slot ? k1 - k0 : 0;
    // the model
    Model M;
    M.m = m;
    uint64_t P = 1, flagged = 0;
    while (P < m) P *= 2;
    uint8_t want = pmt::kOk;
    Hash root{};
    if (m == 0) {
      want = pmt::kNoLeaves;
    } else {
      for (uint64_t i = 0; i < P; i++) {
        Hash h{};
        if (i < m) std::memcpy(h.data(), hashes.p.get() + (l0 + i) * 8, 32);
        M.leaves.push_back(h);
        if (i < m && include.p[l0 + i]) M.include.insert(h), flagged++;
      }
      root = M.rec(0, P).first;
      if (M.used != flagged) want = pmt::kHashesNotInTree;
      else if (cap < 2 * P - 1) want = pmt::kSlotTooSmall;
    }
    const uint8_t got = txst.p[t];
    st.status[got & 15]++;
    if (got != want) {
      fprintf(stderr, "lane %llu (m %llu, cap %llu): status %u, the model %u\n", (unsigned long long)t,
              (unsigned long long)m, (unsigned long long)cap, got, want);
      return false;
    }
    uint8_t idb[32];
    for (int k = 0; k < 8; k++)
      for (int q = 0; q < 4; q++) idb[4 * k + q] = (uint8_t)(root[k] >> (24 - 8 * q));
    if (std::memcmp(idb, txid.p.get() + t * 32, 32) != 0) {
      fprintf(stderr, "lane %llu (m %llu): id differs\n", (unsigned long long)t, (unsigned long long)m);
      return false;
    }
    const uint64_t n = cnt.p[t];
    if (n != (want == pmt::kOk ? M.toks.size() : 0) || n > cap) {
      fprintf(stderr, "lane %llu (m %llu): %llu tokens, the model %zu\n", (unsigned long long)t,
              (unsigned long long)m, (unsigned long long)n, M.toks.size());
      return false;
    }
    st.tokens += n;
    for (uint64_t k = 0; k < n; k++) {
      const Tok& w = M.toks[k];
      bool same = tok.p[k0 + k] == w.kind;
      if (same && w.kind != pmt::kTokNode) {
        uint8_t hb[32];
        for (int x = 0; x < 8; x++)
          for (int q = 0; q < 4; q++) hb[4 * x + q] = (uint8_t)(w.h[x] >> (24 - 8 * q));
        same = std::memcmp(hb, tok_hash.p.get() + (k0 + k) * 32, 32) == 0;
      }
      if (!same) {
        fprintf(stderr, "lane %llu (m %llu): token %llu differs\n", (unsigned long long)t, (unsigned long long)m,
                (unsigned long long)k);
        return false;
      }
    }
    // nothing outside the lane's tokens changed (a failed lane: nothing at all)
    for (uint64_t k = 0; k < nt; k++) {
      if (slot && k >= k0 && k < k0 + n) continue;
      if (tok.p[k] != tok_before[k] || std::memcmp(tok_hash.p.get() + k * 32, hash_before.data() + k * 32, 32) != 0) {
        fprintf(stderr, "lane %llu (m %llu): wrote entry %llu outside its tokens\n", (unsigned long long)t,
                (unsigned long long)m, (unsigned long long)k);
        return false;
      }
    }
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: pmt_build_fuzz ROUNDS RNG_SEED\n");
    return 2;
  }
  const uint64_t rounds = strtoull(argv[1], nullptr, 10);
  Rng r{strtoull(argv[2], nullptr, 10)};
  g_zero[0] = Hash{};
  for (int j = 1; j < 64; j++) mix(g_zero[j].data(), g_zero[j - 1].data(), g_zero[j - 1].data());
  // the bound itself: exact at the edges, rejected where it does not fit
  uint64_t need = 0;
  const uint64_t top = 1ull << 62;
  if (!pmt::slot_bound(top, &need) || need != 2 * top - 1 || pmt::slot_bound(top + 1, &need) ||
      pmt::slot_bound(UINT64_MAX, &need) || !pmt::slot_bound(0, &need) || need != 0 || !pmt::slot_bound(5, &need) ||
      need != 15) {
    fprintf(stderr, "slot_bound edges\n");
    return 1;
  }
  Stats st;
  for (uint64_t i = 0; i < rounds; i++)
    if (!round(r, st)) return 1;
  printf("{\"rounds\": %llu, \"batches\": %llu, \"invalid\": %llu, \"lanes\": %llu, \"tokens\": %llu, "
         "\"status_0\": %llu, \"status_6\": %llu, \"status_12\": %llu, \"status_13\": %llu}\n",
         (unsigned long long)rounds, (unsigned long long)st.batches, (unsigned long long)st.invalid,
         (unsigned long long)st.lanes, (unsigned long long)st.tokens, (unsigned long long)st.status[0],
         (unsigned long long)st.status[6], (unsigned long long)st.status[12], (unsigned long long)st.status[13]);
  return 0;
}
