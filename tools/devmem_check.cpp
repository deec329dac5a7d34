// What a Device owns (corda_amd/csrc/runtime.hpp: the visit of its buffers, fences,
// events and streams; Device::bind, release_idle and the destructor) against
// counting fakes of the HIP calls that code links to -- host only, no GPU:
// tests/test_devmem.py builds this with g++ -fsanitize=address,undefined and runs it.
//  a  the visit reaches every DevBuf / PinBuf / event / stream the structs hold
//     (sizeof of each struct = the bytes visited + its plain members)
//  b  the idle release leaves exactly the kept buffers, and the account equals them
//  c  after ~Device nothing is live and the account is zero (ASan: no leak either)
//  d  the same for a half-initialised Device (hipMalloc failing midway, null events)
//  e  two Devices charge the accounts of their own ids, whatever hipGetDevice says
//  f  the signer's key table and the verification keys' tables (SignKeys, VerifyKeys:
//     not part of Device::visit, so the idle release is never offered them) are bound
//     with the device, survive the idle release with their bytes still in the account,
//     and are freed by ~Device
// prints one JSON line; exit status 1 and a message on the first failed check
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>

#include "../corda_amd/csrc/runtime.hpp"

using namespace cordahip::rt;

namespace {
struct Fakes {
  std::map<void*, size_t> dev, pin;
  std::set<void*> events, streams;
  long mallocs = 0, fail_malloc_at = -1;  // the fail_malloc_at-th hipMalloc from now fails
  int set_device = -1;
  void* handle() { return ::operator new(1); }
  bool clean() const { return dev.empty() && pin.empty() && events.empty() && streams.empty(); }
} g;

void fail(const char* what) {
  fprintf(stderr, "devmem_check: %s\n", what);
  exit(1);
}
#define CHECK(x) \
  if (!(x)) fail(#x)
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  if (g.mallocs++ == g.fail_malloc_at) return hipErrorOutOfMemory;
  *p = g.handle();
  g.dev[*p] = bytes;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  CHECK(g.dev.erase(p) == 1);
  ::operator delete(p);
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) {
  *p = g.handle();
  g.pin[*p] = bytes;
  return hipSuccess;
}
hipError_t hipHostFree(void* p) {
  CHECK(g.pin.erase(p) == 1);
  ::operator delete(p);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  *e = static_cast<hipEvent_t>(g.handle());
  g.events.insert(*e);
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  CHECK(g.events.erase(e) == 1);
  ::operator delete(e);
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
  CHECK(g.events.count(e) == 1);
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  CHECK(g.streams.erase(s) == 1);  // an alias destroyed twice fails here
  ::operator delete(s);
  return hipSuccess;
}
hipError_t hipSetDevice(int id) {
  g.set_device = id;
  return hipSuccess;
}
hipError_t hipGetDevice(int* id) {  // nothing may ask: the answer is another device's
  *id = 0;
  return hipSuccess;
}
}
// a Device's pool is never created here
cordahip::rt::HostPool::~HostPool() {}

namespace {
struct Count : Visitor {
  size_t ndev = 0, npin = 0, nfence = 0, nevent = 0, nstream = 0;
  void dev(DevBuf&, bool) { ndev++; }
  void pin(PinBuf&, bool) { npin++; }
  void fence(Fence&) { nfence++; }
  void event(hipEvent_t&, bool) { nevent++; }
  void stream(hipStream_t&) { nstream++; }
  size_t bytes() const {
    return ndev * sizeof(DevBuf) + npin * sizeof(PinBuf) + nfence * sizeof(Fence) + nevent * sizeof(hipEvent_t) +
           nstream * sizeof(hipStream_t);
  }
};
// a: sizeof(T) is what the visit reached plus `plain` bytes of other members, so a
// buffer or event added to T and not visited fails here (a plain member added: raise
// `plain` by its size)
template <class T>
Count visited(T& t, size_t plain, const char* name) {
  Count c;
  t.visit(c);
  if (sizeof(T) != c.bytes() + plain) {
    fprintf(stderr, "devmem_check: %s: sizeof %zu, visited %zu + plain %zu -- a member is not visited?\n", name,
            sizeof(T), c.bytes(), plain);
    exit(1);
  }
  return c;
}

// the plain members of the structs that have some (bool: with its padding)
constexpr size_t kPackPlain = 8 /* pending */ + 3 * sizeof(uint64_t);
// the lane lists (ed, ec, rsa), a and b, rsa_rows, direct, pending
constexpr size_t kBatchPlain =
    3 * sizeof(std::vector<uint64_t>) + 3 * sizeof(uint64_t) + 8 /* direct */ + 8 /* pending */;
constexpr size_t kTxSetPlain = sizeof(uint32_t*) /* kryo_usage_dev */ + kTxStages * kBatchPlain;

struct Grow : Visitor {  // every buffer a few bytes, every event and stream created
  size_t k = 0;
  bool events = true;
  void dev(DevBuf& b, bool) { (void)b.ensure(8 + k++ % 5); }
  void pin(PinBuf& b, bool) { (void)b.ensure(8 + k++ % 5); }
  void fence(Fence& f) {
    if (events) (void)f.create();
  }
  void event(hipEvent_t& e, bool) {
    if (events && !e) (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
  }
  void stream(hipStream_t& s) {
    if (!events || s) return;
    s = static_cast<hipStream_t>(g.handle());
    g.streams.insert(s);
  }
};
struct Kept : Visitor {
  std::set<void*> devs, pins;
  uint64_t bytes = 0;
  void dev(DevBuf& b, bool keep) {
    CHECK(keep ? b.p && b.cap : !b.p && !b.cap);
    if (keep) devs.insert(b.p), bytes += b.cap;
  }
  void pin(PinBuf& b, bool keep) {
    CHECK(keep ? b.p && b.cap : !b.p && !b.cap);
    if (keep) pins.insert(b.p);
  }
};
template <class M>
std::set<void*> keys(const M& m) {
  std::set<void*> s;
  for (const auto& kv : m) s.insert(kv.first);
  return s;
}
}  // namespace

int main() {
  // a: each struct on its own, then the whole Device
  size_t ndev, npin, nev;
  {
    TxWork tw;
    StreamStage ss;
    PackStage ps;
    BatchStage bs;
    TxSet ts;
    EcWork ew;
    RsaWork rw;
    SignKeys sk;
    visited(sk, 0, "SignKeys");
    EcSignKeys esk;
    visited(esk, sizeof(CurveBook<cordahip::kSignKeySlots>) /* book */, "EcSignKeys");
    static_assert(sizeof(CurveBook<cordahip::kSignKeySlots>) == 4 * sizeof(uint32_t) + cordahip::kSignKeySlots,
                  "built, live and a byte per slot");
    RsaSignKeys rsk;
    visited(rsk, cordahip::kSignKeySlots /* rec_of */ + 64 /* used */, "RsaSignKeys");
    VerifyKeys vk;
    visited(vk, sizeof(uint64_t) /* live */, "VerifyKeys");
    EcVerifyKeys ek;
    visited(ek, sizeof(CurveBook<cordahip::kVkeySlots>) /* book */, "EcVerifyKeys");
    RsaVerifyKeys rk;
    visited(rk, sizeof(uint64_t) /* live */, "RsaVerifyKeys");
    KeyedStage ks;
    visited(ks, sizeof(std::mutex) /* mu */, "KeyedStage");
    visited(tw, 0, "TxWork");
    visited(ss, 0, "StreamStage");
    visited(ps, kPackPlain, "PackStage");
    visited(bs, kBatchPlain, "BatchStage");
    visited(ts, kTxSetPlain, "TxSet");
    visited(ew, 0, "EcWork");
    visited(rw, 0, "RsaWork");
    SigPackWork sp;
    visited(sp, 0, "SigPackWork");
  }
  auto* d = new Device;
  d->bind(3);
  {
    // Device's plain members: ids, placement, pool, budget and workspace sizes, activity,
    // the mutexes and condition variable, turn counters, ring generations, set_busy,
    // s_ec2 (an alias), the encoder's flags and counters; the signer's mutex, its chunk
    // stage's and its key table, which has a visit of its own (f)
    // and the verification keys' mutex, their chunk stage's and their tables, visited with the signer's (f)
    // and the registered ECDSA keys' tables with what the host knows of them (f)
    // and the three routing switches (route_on, ec_route_on, rsa_route_on: each padded to 8 bytes)
    // and the ECDSA signer's table with what the host knows of it (f)
    // and the registered RSA keys' table (f)
    // and the RSA signer's table with what the host knows of it (f)
    // and the mixed-scheme device calls' mutex (sigpack_mu; their scratch is visited)
    constexpr size_t kDeviceOwnPlain = 1288 + 2 * sizeof(std::mutex) + sizeof(SignKeys) + 2 * sizeof(std::mutex) +
                                       sizeof(VerifyKeys) + sizeof(EcVerifyKeys) + 24 + sizeof(EcSignKeys) +
                                       sizeof(RsaVerifyKeys) + sizeof(RsaSignKeys) + sizeof(std::mutex);
    const Count c = visited(*d, kDeviceOwnPlain + kTxSets * kTxSetPlain + kPackStages * kPackPlain, "Device");
    ndev = c.ndev, npin = c.npin, nev = c.nfence + c.nevent;
    CHECK(c.nstream == 7);
  }
  Grow grow;
  d->visit(grow);
  d->s_ec2 = d->s_idcopy;  // as ensure_streams leaves them
  CHECK(g.dev.size() == ndev && g.pin.size() == npin && g.events.size() == nev && g.streams.size() == 7);
  uint64_t all = 0;
  for (const auto& kv : g.dev) all += kv.second;
  CHECK(mem_acct(3).in_use.load() == all && mem_acct(3).peak.load() == all);
  // b: the idle release
  d->release_idle();
  Kept kept;
  d->visit(kept);
  CHECK(kept.devs.size() == 3 + 2 + 1);  // the fixed tables, the ECDSA counters, the encoder's table
  CHECK(keys(g.dev) == kept.devs && keys(g.pin) == kept.pins);
  CHECK(mem_acct(3).in_use.load() == kept.bytes);
  CHECK(g.events.size() == nev && g.streams.size() == 7);  // events and streams stay
  d->visit(grow);  // and the device works again
  CHECK(g.dev.size() == ndev && g.pin.size() == npin);
  // c: destruction
  g.set_device = -1;
  delete d;
  CHECK(g.set_device == 3 && g.clean() && mem_acct(3).in_use.load() == 0);
  // d: half-initialised -- no events or streams, the 40th hipMalloc fails
  d = new Device;
  d->bind(4);
  grow.events = false;
  g.mallocs = 0;
  g.fail_malloc_at = 40;
  d->visit(grow);
  g.fail_malloc_at = -1;
  CHECK(g.dev.size() == ndev - 1 && g.events.empty() && g.streams.empty());
  delete d;
  CHECK(g.clean() && mem_acct(4).in_use.load() == 0);
  delete new Device;  // never bound, nothing allocated
  CHECK(g.clean());
  // e: two devices, two accounts; hipGetDevice's answer (0) gets nothing
  {
    Device a, b;
    a.bind(3);
    b.bind(5);
    (void)a.btab.ensure(1000);
    (void)b.btab.ensure(10);
    (void)b.cover_stack.ensure(7);
    CHECK(mem_acct(3).in_use.load() == 1000 && mem_acct(5).in_use.load() == 17 && mem_acct(0).in_use.load() == 0);
  }
  CHECK(g.clean() && mem_acct(3).in_use.load() == 0 && mem_acct(5).in_use.load() == 0);
  // f: the key table
  {
    auto* k = new Device;
    k->bind(6);
    CHECK(k->keys.tab.dev == 6);
    Grow gk;
    k->visit(gk);
    const size_t before = g.dev.size();
    k->visit_keys(gk);
    size_t nsign = 0, nver = 0;  // visit_keys is the two walks of the families
    k->signer_keys([&](auto&) { nsign++; });
    k->verify_keys([&](auto&) { nver++; });
    CHECK(nsign == 3 && nver == 3);
    // the six tables and the routed lanes' counters (route_tot of VerifyKeys, EcVerifyKeys, RsaVerifyKeys)
    CHECK(g.dev.size() == before + 9 && k->keys.tab.p && k->keys.stage.p && k->keys.ev.ev);
    CHECK(k->ec_keys.tab.dev == 6 && k->ec_keys.tab.p && k->ec_keys.stage.p && k->ec_keys.ev.ev);
    CHECK(k->rsa_keys.tab.dev == 6 && k->rsa_keys.tab.p && k->rsa_keys.stage.p && k->rsa_keys.ev.ev);
    CHECK(k->vkeys.route_tot.dev == 6 && k->vkeys.route_tot.p);
    CHECK(k->ec_vkeys.route_tot.dev == 6 && k->ec_vkeys.route_tot.p);
    CHECK(k->rsa_vkeys.route_tot.dev == 6 && k->rsa_vkeys.route_tot.p);
    CHECK(k->vkeys.tab.dev == 6 && k->vkeys.tab.p && k->vkeys.stage.p && k->vkeys.ev.ev);
    CHECK(k->ec_vkeys.tab.dev == 6 && k->ec_vkeys.tab.p && k->ec_vkeys.stage.p && k->ec_vkeys.ev.ev);
    void *tab = k->keys.tab.p, *stage = k->keys.stage.p, *vtab = k->vkeys.tab.p, *vstage = k->vkeys.stage.p;
    void *etab = k->ec_vkeys.tab.p, *estage = k->ec_vkeys.stage.p;
    void *stab = k->ec_keys.tab.p, *sstage = k->ec_keys.stage.p;
    CHECK(k->rsa_vkeys.tab.dev == 6 && k->rsa_vkeys.tab.p && k->rsa_vkeys.stage.p && k->rsa_vkeys.ev.ev);
    void *rtab = k->rsa_vkeys.tab.p, *rstage = k->rsa_vkeys.stage.p;
    void *rstab = k->rsa_keys.tab.p, *rsstage = k->rsa_keys.stage.p;
    k->release_idle();
    CHECK(k->rsa_keys.tab.p == rstab && k->rsa_keys.stage.p == rsstage && g.dev.count(rstab) && g.pin.count(rsstage));
    CHECK(k->rsa_vkeys.tab.p == rtab && k->rsa_vkeys.stage.p == rstage && g.dev.count(rtab) && g.pin.count(rstage));
    CHECK(k->ec_keys.tab.p == stab && k->ec_keys.stage.p == sstage && g.dev.count(stab) && g.pin.count(sstage));
    CHECK(k->keys.tab.p == tab && k->keys.stage.p == stage && g.dev.count(tab) && g.pin.count(stage));
    CHECK(k->vkeys.tab.p == vtab && k->vkeys.stage.p == vstage && g.dev.count(vtab) && g.pin.count(vstage));
    CHECK(k->ec_vkeys.tab.p == etab && k->ec_vkeys.stage.p == estage && g.dev.count(etab) && g.pin.count(estage));
    Kept kk;
    k->visit(kk);  // what the release walks: the same kept buffers as in b
    CHECK(kk.devs.size() == kept.devs.size());
    CHECK(mem_acct(6).in_use.load() ==
          kk.bytes + k->keys.tab.cap + k->ec_keys.tab.cap + k->vkeys.tab.cap + k->vkeys.route_tot.cap +
              k->ec_vkeys.tab.cap + k->ec_vkeys.route_tot.cap + k->rsa_vkeys.tab.cap + k->rsa_vkeys.route_tot.cap +
              k->rsa_keys.tab.cap);
    delete k;
    CHECK(g.clean() && mem_acct(6).in_use.load() == 0);
  }
  printf("{\"dev_bufs\": %zu, \"pin_bufs\": %zu, \"events\": %zu, \"streams\": 7, \"kept_dev_bufs\": %zu}\n", ndev, npin,
         nev, kept.devs.size());
  return 0;
}
