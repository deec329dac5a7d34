// Mutation fuzzing of cordahip_ecdsa_sign's CSR validation and chunk packing on the
// host, built with ASan + UBSan by tests/test_ecdsa_sign_csr_fuzz.py (no HIP, no
// device), as tools/sign_csr_fuzz.cpp does for cordahip_sign: ECDSA signing batches
// (cordahip_ecdsa_sign_batch: 72-byte signature slots and their lengths out) whose
// every array sits in a heap block of exactly its declared
// entries; msg_off entries, msg_bytes and n are mutated; check_sign_batch
// (csr_check.hpp) must reject exactly the batches the contract rejects (an offset
// that decreases, a last offset past msg_bytes); a batch it accepts is walked as
// cordahip_ecdsa_sign walks it -- chunk by chunk through msg_chunk_layout /
// sign_pack_rows (pack_rows.hpp) into stages of exactly the bytes the layout asks
// for -- so a read outside a caller buffer or a write outside a stage is a
// sanitizer report. The packed rows are compared with the caller's lanes.
// Usage: ecdsa_sign_csr_fuzz <batches> <seed>; prints one JSON line, exit 0 = pass.
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

// the contract, restated: offsets [0, n] non-decreasing, the last within msg_bytes,
// no message of 2^32 bytes or more
bool contract_ok(const uint64_t* off, uint64_t n, uint64_t msg_bytes) {
  if (n == 0) return true;
  for (uint64_t i = 0; i < n; i++)
    if (off[i] > off[i + 1] || off[i + 1] - off[i] > 0xffffffffull) return false;
  return off[n] <= msg_bytes;
}

struct Stats {
  uint64_t batches = 0, invalid = 0, lanes_packed = 0, dense_chunks = 0, csr_chunks = 0, empty_msgs = 0;
};

// the walk of an accepted batch: cordahip_ecdsa_sign's chunk loop with exact-size stages
bool walk(const cordahip_ecdsa_sign_batch& b, uint64_t chunk, Stats& st) {
  for (uint64_t a = 0; a < b.n; a += chunk) {
    const uint64_t m = b.n - a < chunk ? b.n - a : chunk;
    Arr<uint64_t> poff, ho;
    Arr<uint32_t> hid, hl;
    Arr<uint8_t> hgate, hm;
    poff.make(m);
    const SignLayout lay = msg_chunk_layout(b.msg_off, a, m, poff.get());  // what keyed_chunks calls
    hid.make(m);
    hgate.make(b.gate ? m : 0);
    hm.make(lay.bytes);
    ho.make(lay.dense ? 0 : m);
    hl.make(lay.dense ? 0 : m);
    // in two pieces, as the host pool splits a chunk
    const uint64_t mid = m / 2;
    sign_pack_rows(&b, a, 0, mid, lay, poff.get(), hid.get(), hgate.get(), hm.get(), ho.get(), hl.get());
    sign_pack_rows(&b, a, mid, m, lay, poff.get(), hid.get(), hgate.get(), hm.get(), ho.get(), hl.get());
    (lay.dense ? st.dense_chunks : st.csr_chunks)++;
    for (uint64_t i = 0; i < m; i++) {
      const uint64_t o = b.msg_off[a + i], len = b.msg_off[a + i + 1] - o;
      const uint64_t p = lay.dense ? i * 32 : ho.p[i];
      if (!lay.dense && (hl.p[i] != len || (p & 15) || p + len > lay.bytes)) return false;
      if (lay.dense && len != 32) return false;
      if (len && std::memcmp(hm.p.get() + p, b.msg + o, len) != 0) return false;
      if (hid.p[i] != b.key_id[a + i] || (b.gate && hgate.p[i] != b.gate[a + i])) return false;
      st.empty_msgs += len == 0;
    }
    st.lanes_packed += m;
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
    Arr<uint64_t> off;
    off.make(n + 1);
    uint64_t x = r.chance(20) ? r.below(9) : 0;  // msg_off[0] need not be 0
    for (uint64_t i = 0; i < n; i++) {
      off.p[i] = x;
      x += ids32 ? 32 : (r.chance(15) ? 0 : r.chance(30) ? 32 : r.below(300));
    }
    off.p[n] = x;
    Arr<uint8_t> msg, gate, sig, sig_len, status;
    Arr<uint32_t> ids;
    msg.make(x + (r.chance(20) ? r.below(5) : 0));
    for (uint64_t i = 0; i < msg.n; i++) msg.p[i] = (uint8_t)r.next();
    ids.make(n);
    for (uint64_t i = 0; i < n; i++) ids.p[i] = (uint32_t)r.next();
    const bool gated = r.chance(50);
    gate.make(gated ? n : 0);
    for (uint64_t i = 0; i < gate.n; i++) gate.p[i] = r.chance(30) ? (uint8_t)(1 + r.below(255)) : 0;
    sig.make(n * 72);
    sig_len.make(n);
    status.make(n);
    cordahip_ecdsa_sign_batch b{};
    b.n = n;
    b.key_id = ids.get();
    b.msg = msg.get();
    b.msg_off = off.get();
    b.gate = gated ? gate.get() : nullptr;
    b.sig = sig.get();
    b.sig_len = sig_len.get();
    b.status = status.get();
    b.msg_bytes = msg.n;
    if (n && r.chance(55)) {  // mutate: an offset, the declared bytes, or the lane count
      switch (r.below(6)) {
        case 0: off.p[r.below(n + 1)] = r.next(); break;
        case 1: off.p[r.below(n + 1)] += 1 + r.below(40); break;
        case 2: {
          uint64_t& v = off.p[r.below(n + 1)];
          v = v > 3 ? v - 1 - r.below(3) : 0;
          break;
        }
        case 3: b.msg_bytes = r.below(msg.n + 1); break;
        case 4: off.p[n] = msg.n + 1 + r.below(1000); break;
        default: b.n = r.below(n + 1); break;  // fewer lanes than the arrays hold: still sound
      }
    }
    st.batches++;
    const bool want = contract_ok(b.msg_off, b.n, b.msg_bytes);
    const bool got = check_sign_batch(SerialPar{}, &b);
    if (want != got) {
      fprintf(stderr, "batch %llu: contract says %d, check_sign_batch says %d\n", (unsigned long long)it, want, got);
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
    }
  }
  printf("{\"batches\": %llu, \"invalid\": %llu, \"lanes_packed\": %llu, \"dense_chunks\": %llu, \"csr_chunks\": %llu, "
         "\"empty_msgs\": %llu, \"ok\": %s}\n",
         (unsigned long long)st.batches, (unsigned long long)st.invalid, (unsigned long long)st.lanes_packed,
         (unsigned long long)st.dense_chunks, (unsigned long long)st.csr_chunks, (unsigned long long)st.empty_msgs,
         ok ? "true" : "false");
  return ok ? 0 : 1;
}
