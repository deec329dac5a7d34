// CPU check of the K22 extraction rule (corda_amd/csrc/txcomp_inputs_core.hpp: what
// cordahip_txcomp_inputs_device's three kernels run), built by
// tests/test_txcomp_inputs_check.py with g++ -fsanitize=address,undefined.
//
// Each round draws a component batch -- items of STATE_REF, TIME_WINDOW and other kinds
// whose lengths and payload offsets are right, wrong or far outside, transaction offsets
// that are in order, reversed or beyond n_items, a tx_status array or none, and a ref_cap
// from 0 to more than needed -- with the items, the payload, the offsets and the output
// rows each in a heap block of exactly their size, so a read or write outside is an ASan
// report. It runs the core's three steps the way the kernels do (scan_tx per transaction,
// place over the running count, copy_tx into the clamped range) and compares every output
// with a plain re-statement of the rule written without the core's helpers; rows of
// d_refs that no transaction owns must keep their fill pattern.
// Exit 0 when every check holds.
//
// usage: txcomp_inputs_check ROUNDS RNG_SEED
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../corda_amd/csrc/txcomp_inputs_core.hpp"

namespace {

using namespace cordahip;

struct Rng {
  uint64_t s;
  uint64_t next() {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t n) { return n ? next() % n : 0; }
};

constexpr int64_t kLim = (int64_t)1 << 62;
constexpr int64_t kMinS = -31557014167219200ll, kMaxS = 31556889864403199ll;

// the re-statement's Instant: exact in 128 bits, then saturated
int64_t plain_ns(int64_t s, int32_t n) {
  const __int128 v = (__int128)s * 1000000000 + n;
  return v > kLim ? kLim : v < -kLim ? -kLim : (int64_t)v;
}

struct Plain {
  std::vector<uint8_t> rows;  // 36 bytes each, as written (at most ref_cap)
  std::vector<uint64_t> off;
  std::vector<int64_t> from, until;
  std::vector<uint8_t> gate;
};

Plain restate(const std::vector<cordahip_kryo_item>& items, const std::vector<uint8_t>& payload,
              const std::vector<uint64_t>& tio, uint64_t ref_cap, const std::vector<uint8_t>* status) {
  Plain p;
  const uint64_t ntx = tio.size() - 1, n = items.size();
  unsigned __int128 start = 0;
  for (uint64_t t = 0; t < ntx; t++) {
    uint64_t i0 = tio[t] < n ? tio[t] : n, i1 = tio[t + 1] < n ? tio[t + 1] : n;
    std::vector<uint8_t> mine;
    int64_t f = INT64_MIN, u = INT64_MIN;
    bool flagged = false;
    int windows = 0;
    for (uint64_t i = i0; i < i1; i++) {
      const uint64_t o = (uint64_t)(uintptr_t)items[i].data, len = items[i].len;
      if (items[i].kind == 16) {
        if (len != 36 || o > payload.size() || payload.size() - o < 36) flagged = true;
        else mine.insert(mine.end(), payload.begin() + o, payload.begin() + o + 36);
      } else if (items[i].kind == 17) {
        windows++;
        if (len != 25 || o > payload.size() || payload.size() - o < 25) {
          flagged = true;
          continue;
        }
        const uint8_t* d = payload.data() + o;
        int64_t s[2];
        int32_t ns[2];
        std::memcpy(&s[0], d + 1, 8), std::memcpy(&ns[0], d + 9, 4), std::memcpy(&s[1], d + 13, 8), std::memcpy(&ns[1], d + 21, 4);
        bool ok = !(d[0] & ~3) && windows == 1;
        for (int q = 0; q < 2; q++)
          if (d[0] & (1 << q)) ok = ok && ns[q] >= 0 && ns[q] <= 999999999 && s[q] >= kMinS && s[q] <= kMaxS;
        if (!ok) {
          flagged = true;
        } else {
          if (d[0] & 1) f = plain_ns(s[0], ns[0]);
          if (d[0] & 2) u = plain_ns(s[1], ns[1]);
        }
      }
    }
    if (flagged) mine.clear(), f = u = INT64_MIN;
    const uint64_t cnt = mine.size() / 36;
    if (start + cnt > ref_cap) flagged = true;
    const uint64_t a = start < ref_cap ? (uint64_t)start : ref_cap, e = start + cnt < ref_cap ? (uint64_t)(start + cnt) : ref_cap;
    p.off.push_back(a);
    p.rows.insert(p.rows.end(), mine.begin(), mine.begin() + (e - a) * 36);
    start += cnt;
    p.from.push_back(f), p.until.push_back(u);
    const uint8_t st = status ? (*status)[t] : 0;
    p.gate.push_back(st ? st : flagged ? 9 : 0);
  }
  p.off.push_back(start < ref_cap ? (uint64_t)start : ref_cap);
  return p;
}

int fail(const char* what, uint64_t round, uint64_t t) {
  std::fprintf(stderr, "txcomp_inputs_check: %s (round %llu, tx %llu)\n", what, (unsigned long long)round,
               (unsigned long long)t);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: txcomp_inputs_check ROUNDS RNG_SEED\n");
    return 2;
  }
  const uint64_t rounds = std::strtoull(argv[1], nullptr, 10);
  Rng r{std::strtoull(argv[2], nullptr, 10)};
  uint64_t txs = 0, flagged = 0, refs = 0, windows = 0, capped = 0;
  for (uint64_t round = 0; round < rounds; round++) {
    const uint64_t n = r.below(48), plen = r.below(8) ? 36 + r.below(600) : r.below(40), ntx = r.below(12);
    std::vector<uint8_t> payload(plen);
    for (auto& b : payload) b = (uint8_t)r.next();
    std::vector<cordahip_kryo_item> items(n);
    const bool wild = r.below(3) == 0;  // a round of mostly well-formed items, or one with many wrong ones
    for (auto& it : items) {
      std::memset(&it, 0, sizeof it);
      const uint64_t k = r.below(10);
      it.kind = k < 5 ? 16 : k < 6 ? 17 : (uint32_t)r.below(22);
      const uint64_t want = it.kind == 17 ? 25 : 36;
      it.len = r.below(wild ? 3 : 48) ? want : r.below(2) ? want - 1 + 2 * r.below(2) : r.next() >> r.below(64);
      uint64_t off = plen >= want ? r.below(plen - want + 1) : 0;
      const uint64_t o = r.below(wild ? 4 : 96);
      if (o == 0) off = plen >= 35 ? plen - 35 : plen;  // one byte short of a row
      if (o == 1) off = plen + r.below(3);
      if (o == 2) off = r.next() >> r.below(64);
      it.data = reinterpret_cast<const uint8_t*>((uintptr_t)off);
      if (it.kind == 17 && it.len == 25 && off + 25 <= plen && r.below(wild ? 2 : 8)) {  // a valid window row
        uint8_t* d = payload.data() + off;
        d[0] = (uint8_t)r.below(4);
        const int64_t s[4] = {1500000000, kMaxS, kMinS, 4611686018ll};
        const int32_t ns[3] = {0, 999999999, 427387904};
        for (int q = 0; q < 2; q++) {
          const int64_t sv = r.below(4) ? s[r.below(4)] : (int64_t)r.below(1ull << 40) - (1ll << 39);
          const int32_t nv = r.below(4) ? ns[r.below(3)] : (int32_t)r.below(1000000000);
          std::memcpy(d + 1 + 12 * q, &sv, 8), std::memcpy(d + 9 + 12 * q, &nv, 4);
        }
      }
    }
    std::vector<uint64_t> tio(ntx + 1);
    uint64_t at = 0;
    for (auto& x : tio) {
      x = at;
      const uint64_t o = r.below(wild ? 6 : 24);
      if (o == 0) x = n + r.below(5);
      if (o == 1) x = r.next() >> r.below(64);
      if (o == 2) x = r.below(n + 1);  // out of order
      at += r.below(9);
    }
    std::vector<uint8_t> status(ntx);
    for (auto& b : status) b = r.below(4) ? 0 : (uint8_t)(1 + r.below(20));
    const bool with_status = r.below(2);
    // the total before clamping, for ref_cap around it
    const Plain whole = restate(items, payload, tio, ~0ull, nullptr);
    const uint64_t total = whole.off[ntx];
    const uint64_t pick = r.below(6);
    const uint64_t ref_cap = pick == 0 ? 0 : pick == 1 ? total : pick == 2 ? (total ? total - 1 : 0) : pick == 3 ? total + 1 + r.below(8)
                                                                                                               : r.below(total + 2);
    const Plain want = restate(items, payload, tio, ref_cap, with_status ? &status : nullptr);

    // exact heap blocks for everything the core reads or writes
    std::unique_ptr<cordahip_kryo_item[]> h_items(new cordahip_kryo_item[n ? n : 1]);
    if (n) std::memcpy(h_items.get(), items.data(), n * sizeof(cordahip_kryo_item));
    std::unique_ptr<uint8_t[]> h_payload(new uint8_t[plen ? plen : 1]);
    if (plen) std::memcpy(h_payload.get(), payload.data(), plen);
    std::unique_ptr<uint64_t[]> h_tio(new uint64_t[ntx + 1]);
    std::memcpy(h_tio.get(), tio.data(), (ntx + 1) * 8);
    std::unique_ptr<uint32_t[]> h_refs(new uint32_t[ref_cap ? ref_cap * txin::kRefWords : 1]);
    for (uint64_t i = 0; i < ref_cap * txin::kRefWords; i++) h_refs[i] = 0xA5A5A5A5u;
    std::unique_ptr<uint64_t[]> h_off(new uint64_t[ntx + 1]);
    std::unique_ptr<int64_t[]> h_from(new int64_t[ntx ? ntx : 1]), h_until(new int64_t[ntx ? ntx : 1]);
    std::unique_ptr<uint8_t[]> h_gate(new uint8_t[ntx ? ntx : 1]);
    const txin::Batch B{h_items.get(), n, plen ? h_payload.get() : nullptr, plen, h_tio.get(), ntx};

    // the count pass, the scan, the copy pass -- in the kernels' order and with their in-place arrays
    for (uint64_t t = 0; t < ntx; t++) {
      const txin::TxScan x = txin::scan_tx(B, t);
      h_off[t] = x.nref, h_from[t] = x.tw_from, h_until[t] = x.tw_until, h_gate[t] = x.flagged;
      flagged += x.flagged, windows += x.tw_from != txin::kAbsent || x.tw_until != txin::kAbsent;
    }
    uint64_t run = 0;
    for (uint64_t t = 0; t < ntx; t++) {
      const uint64_t c = h_off[t];
      uint8_t g;
      h_off[t] = txin::place(run, c, h_gate[t] != 0, ref_cap, with_status ? status[t] : 0, g);
      h_gate[t] = g;
      run = txin::add_sat(run, c);
    }
    h_off[ntx] = run < ref_cap ? run : ref_cap;
    capped += run > ref_cap;
    for (uint64_t t = 0; t < ntx; t++)
      if (h_off[t + 1] > h_off[t]) txin::copy_tx(B, t, h_refs.get() + h_off[t] * txin::kRefWords, h_off[t + 1] - h_off[t]);

    for (uint64_t t = 0; t <= ntx; t++)
      if (h_off[t] != want.off[t]) return fail("tx_ref_off", round, t);
    for (uint64_t t = 0; t < ntx; t++) {
      if (h_from[t] != want.from[t] || h_until[t] != want.until[t]) return fail("window", round, t);
      if (h_gate[t] != want.gate[t]) return fail("gate", round, t);
    }
    if (want.rows.size() != h_off[ntx] * 36) return fail("row count", round, 0);
    if (!want.rows.empty() && std::memcmp(h_refs.get(), want.rows.data(), want.rows.size()) != 0)
      return fail("rows", round, 0);
    for (uint64_t i = h_off[ntx] * txin::kRefWords; i < ref_cap * txin::kRefWords; i++)
      if (h_refs[i] != 0xA5A5A5A5u) return fail("a row beyond the total was written", round, 0);
    txs += ntx, refs += h_off[ntx];
  }
  std::printf("{\"rounds\": %llu, \"txs\": %llu, \"flagged\": %llu, \"refs\": %llu, \"windows\": %llu, \"capped\": %llu}\n",
              (unsigned long long)rounds, (unsigned long long)txs, (unsigned long long)flagged,
              (unsigned long long)refs, (unsigned long long)windows, (unsigned long long)capped);
  return 0;
}
