// Mutation fuzzing of cordahip_verify_keyed's CSR validation and chunk packing on the
// host, built with ASan + UBSan by tests/test_vkey_csr_fuzz.py (no HIP, no device):
// keyed batches whose every array sits in a heap block of exactly its declared entries;
// sig_off and msg_off entries, sig_bytes, msg_bytes and n are mutated;
// check_keyed_sig_batch (csr_check.hpp) must reject exactly the batches the contract
// rejects (an offset that decreases, a last offset past its *_bytes); a batch it accepts
// is walked as cordahip_verify_keyed walks it -- chunk by chunk through msg_chunk_layout
// / keyed_pack_rows (pack_rows.hpp) into stages of exactly the bytes the layout asks for
// -- so a read outside a caller buffer or a write outside a stage is a sanitizer report.
// The packed rows and the host-decided statuses are compared with the caller's lanes.
// Every accepted batch is then walked as cordahip_rsa_verify_keyed walks it: each lane
// gets a random width class or none (an unknown id), each class's lanes go in launches of
// a small random size through rsa_keyed_msg_offsets / rsa_keyed_pack_rows into exact-size
// stages, and every row is compared with its lane.
// Usage: vkey_csr_fuzz <batches> <seed>; prints one JSON line, exit 0 = pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../corda_amd/csrc/csr_check.hpp"
#include "../corda_amd/csrc/pack_rows.hpp"

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
  void make(uint64_t k) {
    n = k;
    p.reset(new T[k ? k : 1]);
    if (k) std::memset(p.get(), 0, sizeof(T) * k);
  }
  T* get() const { return p.get(); }
};

struct SerialPar {
  template <class F>
  void operator()(uint64_t n, uint64_t, F&& fn) const {
    if (n) fn(0, n);
  }
};

// the contract, restated: both offset arrays [0, n] non-decreasing, the last within its
// *_bytes, no message of 2^32 bytes or more
bool contract_ok(const cordahip_keyed_sig_batch& b) {
  if (b.n == 0) return true;
  for (uint64_t i = 0; i < b.n; i++) {
    if (b.sig_off[i] > b.sig_off[i + 1]) return false;
    if (b.msg_off[i] > b.msg_off[i + 1] || b.msg_off[i + 1] - b.msg_off[i] > 0xffffffffull) return false;
  }
  return b.sig_off[b.n] <= b.sig_bytes && b.msg_off[b.n] <= b.msg_bytes;
}

struct Stats {
  uint64_t batches = 0, invalid = 0, lanes_packed = 0, dense_chunks = 0, csr_chunks = 0, empty_msgs = 0, pre_ok = 0,
           pre_empty = 0, pre_malformed = 0;
  uint64_t rsa_rows[3] = {0, 0, 0}, rsa_launches = 0, rsa_unknown = 0, rsa_oversize = 0, rsa_empty_msgs = 0,
           rsa_edge_lens = 0;
};

// the walk of an accepted batch: cordahip_verify_keyed's chunk loop with exact-size stages
bool walk(const cordahip_keyed_sig_batch& b, uint64_t chunk, Stats& st) {
  const bool do_verify = !(b.flags & CORDAHIP_FLAG_IS_VALID);
  for (uint64_t a = 0; a < b.n; a += chunk) {
    const uint64_t m = b.n - a < chunk ? b.n - a : chunk;
    Arr<uint64_t> poff, ho;
    Arr<uint32_t> hid, hl;
    Arr<uint8_t> hsig, hpre, hm;
    poff.make(m);
    const SignLayout lay = msg_chunk_layout(b.msg_off, a, m, poff.get());
    hid.make(m);
    hsig.make(m * 64);
    hpre.make(m);
    hm.make(lay.bytes);
    ho.make(lay.dense ? 0 : m);
    hl.make(lay.dense ? 0 : m);
    // in two pieces, as the host pool splits a chunk
    const uint64_t mid = m / 2;
    keyed_pack_rows(&b, a, 0, mid, lay, poff.get(), hid.get(), hsig.get(), hpre.get(), hm.get(), ho.get(), hl.get());
    keyed_pack_rows(&b, a, mid, m, lay, poff.get(), hid.get(), hsig.get(), hpre.get(), hm.get(), ho.get(), hl.get());
    (lay.dense ? st.dense_chunks : st.csr_chunks)++;
    static const uint8_t zero[64] = {0};
    for (uint64_t i = 0; i < m; i++) {
      const uint64_t o = b.msg_off[a + i], len = b.msg_off[a + i + 1] - o;
      const uint64_t so = b.sig_off[a + i], sl = b.sig_off[a + i + 1] - so;
      const uint64_t p = lay.dense ? i * 32 : ho.p[i];
      if (!lay.dense && (hl.p[i] != len || (p & 15) || p + len > lay.bytes)) return false;
      if (lay.dense && len != 32) return false;
      if (len && std::memcmp(hm.p.get() + p, b.msg + o, len) != 0) return false;
      if (hid.p[i] != b.key_id[a + i]) return false;
      const uint8_t want = do_verify && (sl == 0 || len == 0) ? CORDAHIP_STATUS_EMPTY
                           : sl != 64                         ? CORDAHIP_STATUS_MALFORMED_SIG
                                                              : CORDAHIP_STATUS_OK;
      if (hpre.p[i] != want) return false;
      if (std::memcmp(hsig.p.get() + i * 64, want == CORDAHIP_STATUS_OK ? b.sig + so : zero, 64) != 0) return false;
      st.empty_msgs += len == 0;
      st.pre_ok += want == CORDAHIP_STATUS_OK;
      st.pre_empty += want == CORDAHIP_STATUS_EMPTY;
      st.pre_malformed += want == CORDAHIP_STATUS_MALFORMED_SIG;
    }
    st.lanes_packed += m;
  }
  return true;
}

// the walk of an accepted batch as cordahip_rsa_verify_keyed's: lanes by width class, a
// launch of at most `launch` rows at a time, exact-size stages filled with a byte no
// packer writes, packed in two pieces as the pool would
bool walk_rsa(const cordahip_keyed_sig_batch& b, Rng& r, Stats& st) {
  std::vector<uint64_t> cl[3];
  for (uint64_t i = 0; i < b.n; i++) {
    const uint64_t k = r.below(4);
    if (k < 3) cl[k].push_back(i);
    else st.rsa_unknown++;  // an id the mirror does not know: not sent
  }
  const uint64_t launch = 1 + r.below(24);
  for (int c = 0; c < 3; c++) {
    const uint32_t W = 64 + 32 * (uint32_t)c;
    const uint64_t slot = 4ull * W;
    for (uint64_t r0 = 0; r0 < cl[c].size(); r0 += launch) {
      const uint64_t rows = cl[c].size() - r0 < launch ? cl[c].size() - r0 : launch;
      const uint64_t* lanes = cl[c].data() + r0;
      Arr<uint64_t> mo;
      mo.make(rows + 1);
      rsa_keyed_msg_offsets(&b, lanes, rows, mo.get());
      Arr<uint32_t> hid;
      Arr<uint8_t> hsig, hm;
      Arr<uint16_t> hsl;
      hid.make(rows);
      hsig.make(rows * slot);
      hsl.make(rows);
      hm.make(mo.p[rows]);
      std::memset(hsig.get(), 0xA5, rows * slot);
      const uint64_t mid = rows / 2;
      rsa_keyed_pack_rows(&b, lanes, W, mo.get(), 0, mid, hid.get(), hsig.get(), hsl.get(), hm.get());
      rsa_keyed_pack_rows(&b, lanes, W, mo.get(), mid, rows, hid.get(), hsig.get(), hsl.get(), hm.get());
      uint64_t sum = 0;
      if (mo.p[0] != 0) return false;
      for (uint64_t q = 0; q < rows; q++) {
        const uint64_t i = lanes[q];
        const uint64_t o = b.msg_off[i], len = b.msg_off[i + 1] - o;
        const uint64_t so = b.sig_off[i], sl = b.sig_off[i + 1] - so;
        if (hid.p[q] != b.key_id[i]) return false;
        if (mo.p[q] != sum || mo.p[q + 1] != sum + len) return false;
        if (len && std::memcmp(hm.get() + sum, b.msg + o, len) != 0) return false;
        sum += len;
        const uint64_t sent = sl <= slot ? sl : 0;  // a signature longer than its slot sends no bytes
        const uint8_t* row = hsig.get() + q * slot;
        if (sent && std::memcmp(row, b.sig + so, sent) != 0) return false;
        for (uint64_t j = sent; j < slot; j++)
          if (row[j]) return false;
        if (hsl.p[q] != (sl < slot + 1 ? sl : slot + 1)) return false;
        st.rsa_oversize += sl > slot;
        st.rsa_empty_msgs += len == 0;
        st.rsa_edge_lens += sl == 0 || sl + 1 == slot || sl == slot || sl == slot + 1;
      }
      if (mo.p[rows] != sum) return false;
      st.rsa_rows[c] += rows;
      st.rsa_launches++;
    }
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t count = argc > 1 ? strtoull(argv[1], nullptr, 10) : 20000;
  Rng r{argc > 2 ? strtoull(argv[2], nullptr, 10) : 1};
  Stats st;
  bool ok = true;
  for (uint64_t it = 0; it < count && ok; it++) {
    const uint64_t n = r.chance(3) ? 0 : 1 + r.below(r.chance(10) ? 700 : 40);
    const bool ids32 = r.chance(35);  // every message a 32-byte id: the dense chunks
    Arr<uint64_t> moff, soff;
    moff.make(n + 1);
    soff.make(n + 1);
    uint64_t x = r.chance(20) ? r.below(9) : 0, y = r.chance(20) ? r.below(9) : 0;  // off[0] need not be 0
    for (uint64_t i = 0; i < n; i++) {
      moff.p[i] = x;
      soff.p[i] = y;
      x += ids32 ? 32 : (r.chance(15) ? 0 : r.chance(30) ? 32 : r.below(300));
      // mostly Ed25519's 64 bytes; one in eight at an RSA slot's edge (4 W - 1, 4 W, 4 W + 1)
      // or well beyond it, for each width class W
      if (r.chance(12)) {
        const uint64_t slot = 4 * (64 + 32 * r.below(3));
        const uint64_t k = r.below(4);
        y += k < 3 ? slot - 1 + k : slot + 2 + r.below(700);
      } else {
        y += r.chance(80) ? 64 : r.chance(30) ? 0 : r.below(130);
      }
    }
    moff.p[n] = x;
    soff.p[n] = y;
    Arr<uint8_t> msg, sig, status;
    Arr<uint32_t> ids;
    Arr<uint64_t> verdict;
    msg.make(x + (r.chance(20) ? r.below(5) : 0));
    for (uint64_t i = 0; i < msg.n; i++) msg.p[i] = (uint8_t)r.next();
    sig.make(y + (r.chance(20) ? r.below(5) : 0));
    for (uint64_t i = 0; i < sig.n; i++) sig.p[i] = (uint8_t)(1 + r.below(255));  // never a zero row by chance
    ids.make(n);
    for (uint64_t i = 0; i < n; i++) ids.p[i] = (uint32_t)r.next();
    status.make(n);
    verdict.make((n + 63) / 64);
    cordahip_keyed_sig_batch b{};
    b.n = n;
    b.key_id = ids.get();
    b.sig = sig.get();
    b.sig_off = soff.get();
    b.msg = msg.get();
    b.msg_off = moff.get();
    b.status = status.get();
    b.verdict = r.chance(70) ? verdict.get() : nullptr;
    b.flags = r.chance(40) ? CORDAHIP_FLAG_IS_VALID : 0;
    b.sig_bytes = sig.n;
    b.msg_bytes = msg.n;
    if (n && r.chance(55)) {  // mutate: an offset of either array, the declared bytes, or the lane count
      Arr<uint64_t>& off = r.chance(50) ? moff : soff;
      const uint64_t bytes = &off == &moff ? msg.n : sig.n;
      switch (r.below(7)) {
        case 0: off.p[r.below(n + 1)] = r.next(); break;
        case 1: off.p[r.below(n + 1)] += 1 + r.below(40); break;
        case 2: {
          uint64_t& v = off.p[r.below(n + 1)];
          v = v > 3 ? v - 1 - r.below(3) : 0;
          break;
        }
        case 3: b.msg_bytes = r.below(msg.n + 1); break;
        case 4: b.sig_bytes = r.below(sig.n + 1); break;
        case 5: off.p[n] = bytes + 1 + r.below(1000); break;
        default: b.n = r.below(n + 1); break;  // fewer lanes than the arrays hold: still sound
      }
    }
    st.batches++;
    const bool want = contract_ok(b);
    const bool got = check_keyed_sig_batch(SerialPar{}, &b);
    if (want != got) {
      fprintf(stderr, "batch %llu: contract says %d, check_keyed_sig_batch says %d\n", (unsigned long long)it, want,
              got);
      ok = false;
      break;
    }
    if (!got) {
      st.invalid++;
      continue;
    }
    const uint64_t chunk = 64 * (1 + r.below(4));  // CORDAHIP_HOST_CHUNK: multiples of 64
    if (!walk(b, chunk, st)) {
      fprintf(stderr, "batch %llu: packed rows differ from the caller's lanes\n", (unsigned long long)it);
      ok = false;
    } else if (!walk_rsa(b, r, st)) {
      fprintf(stderr, "batch %llu: packed RSA rows differ from the caller's lanes\n", (unsigned long long)it);
      ok = false;
    }
  }
  printf("{\"batches\": %llu, \"invalid\": %llu, \"lanes_packed\": %llu, \"dense_chunks\": %llu, \"csr_chunks\": %llu, "
         "\"empty_msgs\": %llu, \"pre_ok\": %llu, \"pre_empty\": %llu, \"pre_malformed\": %llu, "
         "\"rsa_rows\": [%llu, %llu, %llu], \"rsa_launches\": %llu, \"rsa_unknown\": %llu, \"rsa_oversize\": %llu, "
         "\"rsa_empty_msgs\": %llu, \"rsa_edge_lens\": %llu, \"ok\": %s}\n",
         (unsigned long long)st.batches, (unsigned long long)st.invalid, (unsigned long long)st.lanes_packed,
         (unsigned long long)st.dense_chunks, (unsigned long long)st.csr_chunks, (unsigned long long)st.empty_msgs,
         (unsigned long long)st.pre_ok, (unsigned long long)st.pre_empty, (unsigned long long)st.pre_malformed,
         (unsigned long long)st.rsa_rows[0], (unsigned long long)st.rsa_rows[1], (unsigned long long)st.rsa_rows[2],
         (unsigned long long)st.rsa_launches, (unsigned long long)st.rsa_unknown, (unsigned long long)st.rsa_oversize,
         (unsigned long long)st.rsa_empty_msgs, (unsigned long long)st.rsa_edge_lens, ok ? "true" : "false");
  return ok ? 0 : 1;
}
