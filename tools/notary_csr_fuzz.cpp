// Mutation fuzzing of cordahip_notary_tearoff_*'s validation on the host, built with
// ASan + UBSan by tests/test_notary_csr_fuzz.py (no HIP, no device): typed tear-off
// batches whose every array sits in a heap block of exactly its declared entries;
// tx_ref_off and tx_tok_off entries, n_refs, ntok, ntx and the NULL pairing of the five
// window arrays are mutated; check_notary_tearoff (csr_check.hpp) must accept exactly
// the batches an independent statement of the contract accepts (both offset arrays
// non-decreasing, their last entries within n_refs / ntok, the window arrays all given
// or all NULL). A batch it accepts then has every leaf it names -- the refs of each
// transaction in list order, then its window -- formed as K21 forms it and run through
// the host instance of the encoder (kryo_core.hpp encode_leaf: counting mode, then into
// an exact-size leaf), so a read outside a caller array is a sanitizer report. Window
// rows mix valid Instants, the ends of their ranges and invalid rows.
// Usage: notary_csr_fuzz <batches> <seed>; prints one JSON line, exit 0 = pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../corda_amd/csrc/csr_check.hpp"
#include "../corda_amd/csrc/kryo_core.hpp"

using namespace cordahip::rt;
namespace kryo = cordahip::kryo;

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
  T* get() const { return p.get(); }
};

struct SerialPar {
  template <class F>
  void operator()(uint64_t n, uint64_t, F&& fn) const {
    if (n) fn(0, n);
  }
};

// the contract, restated
bool csr_contract(const std::vector<uint64_t>& off, uint64_t ntx, uint64_t limit) {
  for (uint64_t t = 0; t < ntx; t++)
    if (off[t] > off[t + 1]) return false;
  return off[ntx] <= limit;
}
bool contract_ok(const std::vector<uint64_t>& roff, const std::vector<uint64_t>& koff, uint64_t ntx, uint64_t n_refs,
                 uint64_t ntok, const bool given[5]) {
  int g = 0;
  for (int i = 0; i < 5; i++) g += given[i];
  if (g != 0 && g != 5) return false;
  if (ntx == 0) return true;
  return csr_contract(roff, ntx, n_refs) && csr_contract(koff, ntx, ntok);
}

struct Stats {
  uint64_t batches = 0, invalid = 0, ran = 0, txs = 0, ref_leaves = 0, window_leaves = 0, bad_windows = 0;
};

// one leaf through the host encoder: its size from the counting mode, then its bytes into
// a block of exactly that size with level buffers of the encoder's own size
bool encode(const cordahip_kryo_item& it, bool& valid) {
  kryo::Kout count(nullptr, 0, nullptr);
  valid = kryo::encode_leaf(count, it);
  if (!valid) return true;
  std::unique_ptr<uint8_t[]> leaf(new uint8_t[count.pos]), levels(new uint8_t[kryo::kLevelBytes]);
  kryo::Kout o(leaf.get(), count.pos, levels.get());
  if (!kryo::encode_leaf(o, it) || o.pos != count.pos) return false;
  const uint64_t lo = it.kind == CORDAHIP_KRYO_STATE_REF ? 173 : 91, hi = it.kind == CORDAHIP_KRYO_STATE_REF ? 177 : 119;
  return count.pos >= lo && count.pos <= hi && std::memcmp(leaf.get(), "corda\0\0\1", 8) == 0;
}

// one offset array and its declared limit (ntx > 0)
void mutate_off(Rng& rng, std::vector<uint64_t>& off, uint64_t& limit, uint64_t ntx) {
  switch (rng.below(5)) {
    case 0:
      off[rng.below(ntx + 1)] = rng.chance(50) ? rng.next() : rng.below(limit + 3);
      break;
    case 1:
      limit = rng.chance(50) ? rng.below(off[ntx] + 1) : off[ntx] ? off[ntx] - 1 : 0;
      break;
    case 2:
      if (ntx > 1) std::swap(off[rng.below(ntx + 1)], off[rng.below(ntx + 1)]);
      break;
    case 3:
      off[ntx] = limit + 1 + rng.below(3);
      break;
    default:
      off[rng.below(ntx + 1)] += 1 + rng.below(4);
      break;
  }
}

bool one(Rng& rng, Stats& st) {
  uint64_t ntx = rng.below(40);
  std::vector<uint64_t> roff(ntx + 1, 0), koff(ntx + 1, 0);
  roff[0] = rng.chance(20) ? rng.below(4) : 0;  // a batch may start inside its arrays
  koff[0] = rng.chance(20) ? rng.below(4) : 0;
  for (uint64_t t = 0; t < ntx; t++) {
    roff[t + 1] = roff[t] + rng.below(6);
    koff[t + 1] = koff[t] + rng.below(8);
  }
  uint64_t n_refs = roff[ntx] + (rng.chance(30) ? rng.below(5) : 0), ntok = koff[ntx] + (rng.chance(30) ? rng.below(5) : 0);
  bool given[5];
  const bool windows = rng.chance(70);
  for (bool& g : given) g = windows;
  // mutations
  if (rng.chance(40)) {
    switch (rng.below(5)) {
      case 0:
        if (ntx) mutate_off(rng, roff, n_refs, ntx);
        break;
      case 1:
        if (ntx) mutate_off(rng, koff, ntok, ntx);
        break;
      case 2: {  // more or fewer transactions than the offsets were built for
        const uint64_t k = rng.below(45);
        roff.resize(k + 1, rng.chance(50) ? roff.back() : rng.below(n_refs + 2));
        koff.resize(k + 1, rng.chance(50) ? koff.back() : rng.below(ntok + 2));
        ntx = k;
        break;
      }
      case 3:
        given[rng.below(5)] ^= true;
        break;
      default:
        for (bool& g : given) g = rng.chance(50);
        break;
    }
  }
  // every array in a block of exactly its declared entries
  Arr<uint64_t> a_roff, a_koff;
  a_roff.from(roff);
  a_koff.from(koff);
  std::vector<cordahip_state_ref> refs(n_refs);
  const uint32_t edges[12] = {0, 1, 63, 64, 8191, 8192, (1u << 20) - 1, 1u << 20, (1u << 27) - 1, 1u << 27, 0x7fffffffu,
                              0xffffffffu};
  for (auto& r : refs) {
    for (auto& x : r.txhash) x = (uint8_t)rng.next();
    r.index = rng.chance(70) ? edges[rng.below(12)] : (uint32_t)rng.next();
  }
  std::vector<uint8_t> flags(ntx), tok(ntok), tokh(ntok * 32), root(ntx * 32);
  std::vector<int64_t> fs(ntx), us(ntx);
  std::vector<int32_t> fn(ntx), un(ntx);
  const int64_t secs[9] = {0, 127, 128, (int64_t)1 << 34, -1, kryo::kInstantMinSecond, kryo::kInstantMaxSecond,
                           kryo::kInstantMinSecond - 1, kryo::kInstantMaxSecond + 1};
  const int32_t nanos[7] = {0, 127, 128, 999999999, 1000000000, -1, INT32_MIN};
  for (uint64_t t = 0; t < ntx; t++) {
    flags[t] = (uint8_t)((rng.chance(60) ? 0x80 : 0) | (rng.chance(90) ? rng.below(4) : rng.below(128)));
    const bool wild = rng.chance(15);  // an invalid second or nano now and then
    fs[t] = secs[rng.below(wild ? 9 : 7)], us[t] = secs[rng.below(wild ? 9 : 7)];
    fn[t] = nanos[rng.below(wild ? 7 : 4)], un[t] = nanos[rng.below(wild ? 7 : 4)];
  }
  Arr<cordahip_state_ref> a_refs;
  Arr<uint8_t> a_flags, a_tok, a_tokh, a_root, a_status;
  Arr<int64_t> a_fs, a_us;
  Arr<int32_t> a_fn, a_un;
  a_refs.from(refs), a_flags.from(flags), a_tok.from(tok), a_tokh.from(tokh), a_root.from(root);
  a_status.from(std::vector<uint8_t>(ntx, 0xee));
  a_fs.from(fs), a_us.from(us), a_fn.from(fn), a_un.from(un);

  cordahip_notary_tearoff_batch b{};
  b.ntx = ntx;
  b.refs = a_refs.get();
  b.tx_ref_off = a_roff.get();
  b.n_refs = n_refs;
  b.tw_flags = given[0] ? a_flags.get() : nullptr;
  b.tw_from_s = given[1] ? a_fs.get() : nullptr;
  b.tw_from_nano = given[2] ? a_fn.get() : nullptr;
  b.tw_until_s = given[3] ? a_us.get() : nullptr;
  b.tw_until_nano = given[4] ? a_un.get() : nullptr;
  b.tok = a_tok.get();
  b.tok_hash = a_tokh.get();
  b.tx_tok_off = a_koff.get();
  b.ntok = ntok;
  b.root = a_root.get();
  b.tx_status = a_status.get();

  st.batches++;
  const bool want = contract_ok(roff, koff, ntx, n_refs, ntok, given);
  const bool got = check_notary_tearoff(SerialPar{}, &b);
  if (want != got) {
    fprintf(stderr, "verdicts differ: contract %d, check_notary_tearoff %d (ntx %llu, n_refs %llu, ntok %llu)\n", (int)want,
            (int)got, (unsigned long long)ntx, (unsigned long long)n_refs, (unsigned long long)ntok);
    return false;
  }
  if (!got) {
    st.invalid++;
    return true;
  }
  // an accepted batch: every leaf it names, as K21 forms its items
  st.ran++;
  st.txs += ntx;
  for (uint64_t t = 0; t < ntx; t++) {
    for (uint64_t i = b.tx_ref_off[t]; i < b.tx_ref_off[t + 1]; i++) {
      cordahip_kryo_item it{};
      it.kind = CORDAHIP_KRYO_STATE_REF;
      it.data = reinterpret_cast<const uint8_t*>(b.refs + i);
      it.len = sizeof(cordahip_state_ref);
      bool valid = false;
      if (!encode(it, valid) || !valid) return false;
      st.ref_leaves++;
    }
    if (!b.tw_flags || !(b.tw_flags[t] & 0x80)) continue;
    std::unique_ptr<uint8_t[]> row(new uint8_t[kryo::kTimeWindowLen]);
    row[0] = b.tw_flags[t] & 0x7f;
    std::memcpy(row.get() + kryo::kTwFromS, &b.tw_from_s[t], 8);
    std::memcpy(row.get() + kryo::kTwFromN, &b.tw_from_nano[t], 4);
    std::memcpy(row.get() + kryo::kTwUntilS, &b.tw_until_s[t], 8);
    std::memcpy(row.get() + kryo::kTwUntilN, &b.tw_until_nano[t], 4);
    cordahip_kryo_item it{};
    it.kind = CORDAHIP_KRYO_TIME_WINDOW;
    it.data = row.get();
    it.len = kryo::kTimeWindowLen;
    bool valid = false;
    if (!encode(it, valid)) return false;
    // the rule of the header, restated
    bool rule = !(row[0] & ~3u);
    const int64_t s[2] = {b.tw_from_s[t], b.tw_until_s[t]};
    const int32_t n[2] = {b.tw_from_nano[t], b.tw_until_nano[t]};
    for (int i = 0; i < 2; i++)
      if (row[0] & (1u << i))
        rule = rule && n[i] >= 0 && n[i] <= 999999999 && s[i] >= -31557014167219200ll && s[i] <= 31556889864403199ll;
    if (rule != valid) return false;
    st.window_leaves += valid;
    st.bad_windows += !valid;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t batches = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
  Rng rng{argc > 2 ? strtoull(argv[2], nullptr, 10) : 1};
  Stats st;
  bool ok = true;
  for (uint64_t i = 0; i < batches && ok; i++) ok = one(rng, st);
  printf("{\"ok\": %s, \"batches\": %llu, \"invalid\": %llu, \"ran\": %llu, \"txs\": %llu, \"ref_leaves\": %llu, "
         "\"window_leaves\": %llu, \"bad_windows\": %llu}\n",
         ok ? "true" : "false", (unsigned long long)st.batches, (unsigned long long)st.invalid,
         (unsigned long long)st.ran, (unsigned long long)st.txs, (unsigned long long)st.ref_leaves,
         (unsigned long long)st.window_leaves, (unsigned long long)st.bad_windows);
  return ok ? 0 : 1;
}
