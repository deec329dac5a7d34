// libcordahip.so per-device runtime: the host pools, the pipeline streams, the
// device-memory budget, the enqueue helpers of the three signature schemes (their
// workspaces and reuse fences), the idle release, and context init / shutdown.
// What a Device owns and how it is released is in runtime.hpp.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "runtime.hpp"
#include "sig_pack.hpp"

using namespace cordahip;
using namespace cordahip::rt;

namespace cordahip {
namespace rt {

// ---- host fork-join pool -----------------------------------------------------
HostPool::HostPool(int nthreads, const std::vector<int>& cpus) {
  for (int i = 1; i < nthreads; i++) {
    threads_.emplace_back([this] { worker(); });
    if (!cpus.empty()) {  // the device's node: its rows are packed next to its GPU
      cpu_set_t cs;
      CPU_ZERO(&cs);
      for (int c : cpus)
        if (c >= 0 && c < CPU_SETSIZE) CPU_SET(c, &cs);
      (void)pthread_setaffinity_np(threads_.back().native_handle(), sizeof(cs), &cs);
    }
  }
}

NodeBind::NodeBind(const Device& d) {
  if (d.place.cpus.empty()) return;
  cpu_set_t old, cs;
  if (pthread_getaffinity_np(pthread_self(), sizeof(old), &old) != 0) return;
  CPU_ZERO(&cs);
  for (int c : d.place.cpus)
    if (c >= 0 && c < CPU_SETSIZE) CPU_SET(c, &cs);
  if (CPU_EQUAL(&cs, &old) || pthread_setaffinity_np(pthread_self(), sizeof(cs), &cs) != 0) return;
  saved_.assign(reinterpret_cast<unsigned char*>(&old), reinterpret_cast<unsigned char*>(&old) + sizeof(old));
  bound_ = true;
}

NodeBind::~NodeBind() {
  if (bound_) (void)pthread_setaffinity_np(pthread_self(), sizeof(cpu_set_t), reinterpret_cast<cpu_set_t*>(saved_.data()));
}

HostPool& pool_of(cordahip_ctx* ctx, Device& d) { return d.pool ? *d.pool : *ctx->host; }

HostPool::~HostPool() {
  {
    std::lock_guard<std::mutex> g(m_);
    stop_ = true;
  }
  cv_.notify_all();
  for (auto& t : threads_) t.join();
}

void HostPool::run_pieces(Job& j) {
  for (;;) {
    const uint64_t k = j.next.fetch_add(1);
    if (k >= j.npieces) return;
    const uint64_t lo = k * j.piece, hi = std::min(j.n, lo + j.piece);
    (*j.fn)(lo, hi);
    if (j.done.fetch_add(1) + 1 == j.npieces) {
      std::lock_guard<std::mutex> g(j.m);
      j.cv.notify_all();
    }
  }
}

void HostPool::worker() {
  for (;;) {
    std::shared_ptr<Job> j;
    {
      std::unique_lock<std::mutex> g(m_);
      for (;;) {
        while (!q_.empty() && q_.front()->next.load() >= q_.front()->npieces) q_.pop_front();  // exhausted
        if (!q_.empty()) {
          j = q_.front();
          break;
        }
        if (stop_) return;
        cv_.wait(g);
      }
    }
    run_pieces(*j);
  }
}

void HostPool::parallel_for(uint64_t n, uint64_t grain, const std::function<void(uint64_t, uint64_t)>& fn) {
  if (n == 0) return;
  grain = std::max<uint64_t>(grain, 1);
  const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>((n + grain - 1) / grain, 4 * (uint64_t)threads()));
  if (want == 1 || threads_.empty()) {
    fn(0, n);
    return;
  }
  auto j = std::make_shared<Job>();
  j->fn = &fn;
  j->n = n;
  j->piece = (n + want - 1) / want;
  j->npieces = (n + j->piece - 1) / j->piece;
  {
    std::lock_guard<std::mutex> g(m_);
    q_.push_back(j);
  }
  cv_.notify_all();
  run_pieces(*j);
  {
    std::unique_lock<std::mutex> g(j->m);
    j->cv.wait(g, [&] { return j->done.load() == j->npieces; });
  }
  std::lock_guard<std::mutex> g(m_);  // drop it if no worker got to pop it
  for (auto it = q_.begin(); it != q_.end(); ++it)
    if (*it == j) {
      q_.erase(it);
      break;
    }
}

// ---- ticket pool ---------------------------------------------------------------
WorkerPool::WorkerPool(int nthreads) {
  for (int i = 0; i < nthreads; i++) threads_.emplace_back([this] { run(); });
}

WorkerPool::~WorkerPool() {
  {
    std::lock_guard<std::mutex> g(m_);
    stop_ = true;
  }
  cv_.notify_all();
  for (auto& t : threads_) t.join();
}

void WorkerPool::push(std::shared_ptr<JobState> st, std::function<int()> fn) {
  {
    std::lock_guard<std::mutex> g(m_);
    q_.emplace_back(std::move(st), std::move(fn));
  }
  cv_.notify_one();
}

void WorkerPool::run() {
  for (;;) {
    std::pair<std::shared_ptr<JobState>, std::function<int()>> job;
    {
      std::unique_lock<std::mutex> g(m_);
      cv_.wait(g, [this] { return stop_ || !q_.empty(); });
      if (q_.empty()) return;  // stop_ and drained: queued jobs always run
      job = std::move(q_.front());
      q_.pop_front();
    }
    int rc;
    try {
      rc = job.second();
    } catch (...) {
      rc = CORDAHIP_ERR_OUT_OF_MEMORY;  // std::bad_alloc from host staging vectors
    }
    {
      std::lock_guard<std::mutex> g(job.first->m);
      job.first->rc = rc;
      job.first->done = true;
    }
    job.first->cv.notify_all();
  }
}

int hip_err(hipError_t e) { return e == hipSuccess ? CORDAHIP_SUCCESS : CORDAHIP_ERR_HIP; }

hipError_t ensure_streams(Device& d) {
  std::lock_guard<std::mutex> g(d.streams_mu);
  if (d.s_copy) return hipSuccess;
  // Every pipeline stream needs a hardware queue of its own: streams sharing a
  // queue serialise, and a copy enqueued early (the tx-id slices' leaf bytes,
  // a C5 chunk waiting for its stage) then holds back every later kernel of the
  // other stream. HIP hands out pool queues (GPU_MAX_HW_QUEUES, 4 on the box)
  // round-robin over every stream of the process, so a 4th pipeline stream
  // shared one with s_ed or s_copy depending on creation order (c4h 45.1 M
  // sigs/s, or C5 84.6 instead of 95.8 M/s: profiles/r03_stream_queues.json). A
  // stream created with a CU mask (here: all CUs) gets a dedicated queue; the
  // ECDSA stream keeps the higher priority, which also gives it a queue of its
  // own (at normal priority it shared s_ed's and the two sections ran back to back).
  int lo = 0, hi = 0, ncu = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
  e = e ? e : hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, d.id);
  std::vector<uint32_t> all((std::max(ncu, 1) + 31) / 32, 0xffffffffu);
  auto dedicated = [&](hipStream_t* st) { return hipExtStreamCreateWithCUMask(st, (uint32_t)all.size(), all.data()); };
  hipStream_t c = nullptr, x = nullptr, y = nullptr, z = nullptr, x2 = nullptr;
  e = e ? e : dedicated(&c);
  e = e ? e : dedicated(&x);
  e = e ? e : hipStreamCreateWithPriority(&y, hipStreamNonBlocking, hi);
  e = e ? e : dedicated(&z);
  e = e ? e : dedicated(&x2);
  if (e != hipSuccess) {
    for (hipStream_t s : {c, x, y, z, x2})
      if (s) (void)hipStreamDestroy(s);
    return e;
  }
  d.s_ed = x;
  d.s_ed2 = x2;
  d.s_ec = y;
  // generic batches' alternate ECDSA chunks run on the id-copy stream, idle in those
  // batches (no sixth hardware queue)
  d.s_ec2 = z;
  d.s_idcopy = z;
  d.s_copy = c;
  return hipSuccess;
}

// Launch-pair sizes of the split kernels = the largest workspace per device.
// Bigger launches pay fewer end-of-grid tails (C2, measured: 2^18 91.5, 2^20
// 93.2, 2^22 96.4, 2^24 97.2 M verifs/s): a 2^24-lane batch runs as ONE
// prep/ladder pair over 41 GB of HBM (14% of the MI355X's 288 GB). Smaller
// batches allocate only what they use (grow-only, from 2^18 lanes up).
constexpr uint64_t kEdWsLanes = 1ull << 24;  // x 2,432 B = 41 GB of Ed25519 workspace at most
constexpr uint64_t kEcWsSlots = 1ull << 24;  // x 1,120 B = 18.8 GB of ECDSA workspace at most
constexpr uint64_t kWsMinLanes = 1ull << 18;

// Workspace-size overrides (multiples of 64): tests use them to force the
// multi-chunk paths (several prep/ladder launch sets per batch) at small sizes.
uint64_t env_lanes(const char* name, uint64_t dflt) {
  const char* v = getenv(name);
  const uint64_t x = v ? strtoull(v, nullptr, 10) : 0;
  return x >= 64 ? x / 64 * 64 : dflt;
}

// The keyed half of a routed ECDSA enqueue (K15; d.ec_mu[slot] held, the slot's scratch
// and perm large enough, s behind the slot's fence): under d.vkey_mu, as every keyed
// call -- behind ec_vkeys.ev, followed by ec_vkeys.ev -- the gather, route and scatter
// passes and K13 over each live curve's run. *routed stays false, and nothing is
// launched, when no ECDSA key is live any more or the counters cannot be allocated:
// the caller then takes the unrouted path, which is always right. count (K24, the mixed
// device call; null for the dense calls): the device's word with the rows below n to route.
static hipError_t ec_route_and_keyed(Device& d, EcWork& w, const uint8_t* scheme, const uint8_t* keys,
                                     const uint8_t* key_len, const uint8_t* sigs, const uint8_t* sig_len,
                                     const uint8_t* msgs, const uint64_t* msg_off, uint32_t msg_len, uint64_t n,
                                     const uint8_t* pre, uint8_t* status, uint32_t flags, hipStream_t s,
                                     bool* routed, const uint32_t* count = nullptr) {
  std::lock_guard<std::mutex> vk(d.vkey_mu);
  const auto& book = d.ec_vkeys.book;
  if (!d.ec_vkeys.tab.p || !book.any_live()) return hipSuccess;
  if (!d.ec_vkeys.route_tot.p) {  // the device's first routed ECDSA enqueue
    if (d.ec_vkeys.route_tot.ensure(16) != hipSuccess) {
      (void)hipGetLastError();
      return hipSuccess;
    }
    const hipError_t z = hipMemsetAsync(d.ec_vkeys.route_tot.p, 0, 16, s);
    if (z != hipSuccess) return z;
  }
  *routed = true;
  const uint32_t* vtab = d.ec_vkeys.tab.as<uint32_t>();
  return fenced({&d.ec_vkeys.ev}, s, [&] {
    const hipError_t e =
        launch_ecdsa_route(scheme, keys, key_len, n, vtab, w.route.as<uint32_t>(), w.counters.as<unsigned int>(),
                           w.perm.as<unsigned int>(), d.ec_vkeys.route_tot.as<unsigned long long>(), s, count);
    return e ? e
             : launch_ecdsa_verify_keyed_idx(w.route.as<uint32_t>(), w.perm.as<unsigned int>(),
                                             w.counters.as<unsigned int>(), n, sigs, sig_len, msgs, msg_off, msg_len,
                                             pre, flags, vtab, book.has_live(CORDAHIP_SCHEME_ECDSA_SECP256K1_SHA256),
                                             book.has_live(CORDAHIP_SCHEME_ECDSA_SECP256R1_SHA256), status, s);
  });
}

// Enqueue ECDSA verification of n slot-layout lanes on stream s (device current,
// d.ec_mu[slot] held): the slot's work buffers are reused only after their previous
// user's kernels (on whatever stream) have finished.
// With ECDSA routing on and a live ECDSA key (K15): gather, route and scatter, K13 over
// each curve's keyed run, K2 over the generic list, the verdict words from the statuses
// -- all on s, no count read back. Lock order: ec_mu[slot], then vkey_mu (Device,
// runtime.hpp); vkey_mu is never held while this function waits for a lock, a fence or
// an allocation.
hipError_t ec_verify_enqueue(Device& d, const uint8_t* scheme, const uint8_t* keys, const uint8_t* key_len,
                             const uint8_t* sigs, const uint8_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off,
                             uint32_t msg_len, uint64_t n, const uint8_t* pre, uint8_t* status,
                             unsigned long long* verdict, uint32_t flags, hipStream_t s, int slot) {
  EcWork& w = d.ec[slot];
  bool want_route = d.ec_route_on.load(std::memory_order_relaxed) && n && n <= ecdsa_route_max_lanes();
  if (want_route) {  // a look at the registry; decided for good in ec_route_and_keyed
    std::lock_guard<std::mutex> vk(d.vkey_mu);
    want_route = d.ec_vkeys.tab.p && d.ec_vkeys.book.any_live();
  }
  // the scratch grows in powers of two from a floor, behind the workspace's fence; no
  // room for it: the batch is verified unrouted
  const size_t sc_bytes = want_route ? ecdsa_route_scratch_bytes(n) : 0;
  // the budget's ECDSA share (cordahip_init); slot 1 serves the host pipelines'
  // alternate chunks and holds at most half of slot 0
  const uint64_t ws_slots = slot ? std::max<uint64_t>(64, d.ec_ws_slots / 2 / 64 * 64) : d.ec_ws_slots;
  const uint64_t slots = std::min<uint64_t>(ws_slots, (std::max<uint64_t>(n, 1) + 63) / 64 * 64);
  const uint64_t perm_bytes = std::max<uint64_t>(n, 1) * 4;
  const bool ws_needed = w.ws.cap < slots * ecdsa_ws_slot_bytes() || w.perm.cap < perm_bytes;
  hipError_t e = w.ev.grow(ws_needed || w.route.cap < sc_bytes, [&] {
    if (ws_needed) {
      const uint64_t want = std::max<uint64_t>(slots, std::min<uint64_t>(ws_slots, kWsMinLanes));
      if (w.ws.ensure(want * ecdsa_ws_slot_bytes()) || w.perm.ensure(perm_bytes)) return hipErrorOutOfMemory;
    }
    if (w.route.cap < sc_bytes && w.route.ensure(sc_bytes) != hipSuccess) {
      (void)hipGetLastError();
      want_route = false;
    }
    return hipSuccess;
  });
  if (e != hipSuccess) return e;
  if (w.counters.ensure(64)) return hipErrorOutOfMemory;
  e = w.ev.wait(s);
  bool routed = false;
  if (e == hipSuccess && want_route)
    e = ec_route_and_keyed(d, w, scheme, keys, key_len, sigs, sig_len, msgs, msg_off, msg_len, n, pre, status, flags,
                           s, &routed);
  if (e == hipSuccess && routed) {
    e = launch_ecdsa_verify_routed(scheme, keys, key_len, sigs, sig_len, msgs, msg_off, msg_len, n,
                                   d.gtab_k1.as<uint32_t>(), d.gtab_r1.as<uint32_t>(), pre, status, verdict,
                                   w.counters.as<unsigned int>(), w.perm.as<unsigned int>(), w.ws.as<uint32_t>(),
                                   w.ws.cap / ecdsa_ws_slot_bytes() / 64 * 64, flags, s);
  } else if (e == hipSuccess) {
    e = launch_ecdsa_verify(scheme, keys, key_len, sigs, sig_len, msgs, msg_off, msg_len, n,
                            d.gtab_k1.as<uint32_t>(), d.gtab_r1.as<uint32_t>(), pre, status, verdict,
                            w.counters.as<unsigned int>(), w.perm.as<unsigned int>(), w.ws.as<uint32_t>(),
                            w.ws.cap / ecdsa_ws_slot_bytes() / 64 * 64, flags, s);
  }
  if (routed) {  // whatever was launched is fenced, also after a failure
    const hipError_t r = w.ev.record(s);
    return e ? e : r;
  }
  return e ? e : w.ev.record(s);
}

// Enqueue RSASSA-PSS verification of n rows of one width class on stream s (device
// current, d.rsa_mu held). The workspace holds at most kRsaWsRows rows (the
// launches loop over it) and is reused only after its previous user's kernels.
constexpr uint64_t kRsaWsRows = 1ull << 17;  // x 518 B (4096-bit rows) = 68 MB at most
// CORDAHIP_RSA_WS_ROWS (a multiple of 64, at least 64; tests): the rows the RSA workspace
// holds at most and a launch takes at most, so that the launch loop runs with a few
// hundred rows. 0: unset, the workspace's own size decides as before.
static uint64_t rsa_ws_rows_env() {
  static const uint64_t v = env_lanes("CORDAHIP_RSA_WS_ROWS", 0);
  return v;
}
// the rows of class W a launch takes from the workspace as it is
static uint64_t rsa_ws_rows(const RsaWork& w, uint32_t W) {
  const uint64_t rows = w.ws.cap / rsa_ws_row_bytes(W) / 64 * 64;
  return rsa_ws_rows_env() ? std::min(rows, rsa_ws_rows_env()) : rows;
}
hipError_t rsa_ws_grow(Device& d, uint32_t W, uint64_t n) {
  RsaWork& w = d.rsa;
  const uint64_t cap = rsa_ws_rows_env() ? rsa_ws_rows_env() : kRsaWsRows;
  const uint64_t rows = std::min<uint64_t>(cap, (std::max<uint64_t>(n, 1) + 63) / 64 * 64);
  const size_t rb = rsa_ws_row_bytes(W);
  return w.ev.grow(w.ws.cap < rows * rb, [&] { return w.ws.ensure(rows * rb) ? hipErrorOutOfMemory : hipSuccess; });
}

// The keyed part of one launch of a routed RSA enqueue (K20; d.rsa_mu held, the
// workspace's scratch large enough, s behind the workspace's fence and the launch's
// prep): under d.vkey_mu, as every keyed call -- behind rsa_vkeys.ev, followed by
// rsa_vkeys.ev -- the route pass and K18's exponentiation over the keyed list. *routed
// stays false, and nothing is launched, when no RSA key is live any more or the
// counters cannot be allocated: the launch then runs unrouted, which is always right.
// launch_count (K24, the mixed device call; null for the dense calls): the device's word
// with the launch's rows below m, as launch_rsa_routed_head left it.
static hipError_t rsa_route_and_keyed(Device& d, const uint32_t* mod, const uint32_t* exp, uint32_t W, uint64_t lo,
                                      uint64_t m, uint64_t ws_rows, uint64_t cap_rows, hipStream_t s, bool* routed,
                                      const unsigned int* launch_count = nullptr) {
  RsaWork& w = d.rsa;
  std::lock_guard<std::mutex> vk(d.vkey_mu);
  RsaVerifyKeys& k = d.rsa_vkeys;
  if (!k.live || !k.tab.p) return hipSuccess;
  if (!k.route_tot.p) {  // the device's first routed RSA enqueue
    if (k.route_tot.ensure(16) != hipSuccess) {
      (void)hipGetLastError();
      return hipSuccess;
    }
    const hipError_t z = hipMemsetAsync(k.route_tot.p, 0, 16, s);
    if (z != hipSuccess) return z;
  }
  *routed = true;
  return fenced({&k.ev}, s, [&] {
    return launch_rsa_routed_keyed(mod, exp, W, lo, m, k.tab.as<uint32_t>(), w.ws.as<uint8_t>(), ws_rows,
                                   w.route.as<uint32_t>(), cap_rows, k.route_tot.as<unsigned long long>(), s,
                                   launch_count);
  });
}

// With RSA routing on and a live RSA key (K20), per launch: the prep, the route pass
// and K18's exponentiation over the keyed list, K8's over the generic list, the check
// -- all on s, no count read back. Lock order: rsa_mu (the caller's), then vkey_mu;
// vkey_mu is never held while this function waits for a lock, a fence or an allocation.
hipError_t rsa_verify_enqueue(Device& d, const uint32_t* mod, const uint32_t* exp, const uint8_t* sigs,
                              const uint16_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off, uint32_t msg_len,
                              uint32_t W, uint64_t n, const uint8_t* pre, uint8_t* status,
                              unsigned long long* verdict, uint32_t flags, hipStream_t s) {
  RsaWork& w = d.rsa;
  bool want_route = d.rsa_route_on.load(std::memory_order_relaxed) && n;
  if (want_route) {  // a look at the registry; decided for good, per launch, in rsa_route_and_keyed
    std::lock_guard<std::mutex> vk(d.vkey_mu);
    want_route = d.rsa_vkeys.live && d.rsa_vkeys.tab.p;
  }
  hipError_t e = rsa_ws_grow(d, W, n);
  if (e != hipSuccess) return e;
  const uint64_t ws_rows = rsa_ws_rows(w, W);
  // the scratch follows the largest launch of this call, behind the workspace's fence; no
  // room for it: the batch is verified unrouted
  const uint64_t cap_rows = std::min<uint64_t>(rsa_launch_rows(ws_rows), (n + 63) / 64 * 64);
  const size_t sc_bytes = want_route ? rsa_route_scratch_bytes(cap_rows) : 0;
  e = w.ev.grow(w.route.cap < sc_bytes, [&] {
    if (w.route.ensure(sc_bytes) != hipSuccess) {
      (void)hipGetLastError();
      want_route = false;
    }
    return hipSuccess;
  });
  e = e ? e : w.ev.wait(s);
  if (e == hipSuccess && !want_route) {
    e = launch_rsa_pss_verify(mod, exp, sigs, sig_len, msgs, msg_off, msg_len, W, n, pre, status, verdict,
                              w.ws.as<uint8_t>(), ws_rows, flags, s);
    return e ? e : w.ev.record(s);
  }
  const uint64_t lr = rsa_launch_rows(ws_rows);
  if (e == hipSuccess && !lr) e = hipErrorInvalidValue;
  bool launched = false;
  for (uint64_t lo = 0; lo < n && e == hipSuccess; lo += lr) {
    const uint64_t m = std::min(lr, n - lo);
    launched = true;
    e = launch_rsa_routed_head(mod, exp, sigs, sig_len, msg_off, msg_len, W, lo, m, pre, w.ws.as<uint8_t>(), ws_rows,
                               flags, s);
    bool routed = false;
    e = e ? e : rsa_route_and_keyed(d, mod, exp, W, lo, m, ws_rows, cap_rows, s, &routed);
    e = e ? e
          : launch_rsa_routed_tail(mod, exp, msgs, msg_off, msg_len, W, lo, m, status, verdict, w.ws.as<uint8_t>(),
                                   ws_rows, w.route.as<uint32_t>(), cap_rows, routed, s);
  }
  if (launched) {  // whatever was launched is fenced, also after a failure
    const hipError_t r = w.ev.record(s);
    return e ? e : r;
  }
  return e;
}

// The Ed25519 workspace of a slot grown for n lanes (d.ed_mu[slot] held); `more`
// ensures what else the caller keeps behind the slot's fence.
template <class G>
static hipError_t ed_ws_grow(Device& d, int slot, uint64_t n, bool more_needed, G&& more) {
  DevBuf& ws = d.ed_ws[slot];
  // the budget's Ed25519 shares (cordahip_init, device_budget): slot 1 only serves the
  // alternating chunks of the pipelines (host batches, streams, signed-tx chunks) and
  // holds at most half of slot 0. The launch loops over whatever the workspace holds,
  // so a smaller one only costs extra launch pairs.
  const uint64_t cap_lanes = d.ed_ws_lanes[slot ? 1 : 0];
  const uint64_t lanes = std::min<uint64_t>(cap_lanes, (std::max<uint64_t>(n, 1) + 63) / 64 * 64);
  const uint64_t lane_bytes = ed25519_ws_lane_bytes();
  const bool ws_needed = ws.cap < lanes * lane_bytes;
  return d.ed_ev[slot].grow(ws_needed || more_needed, [&] {
    if (!ws_needed) return more();
    uint64_t want = std::max<uint64_t>(lanes, std::min<uint64_t>(cap_lanes, kWsMinLanes));
    const uint64_t had = ws.cap / lane_bytes / 64 * 64;  // ensure() frees it before allocating
    hipError_t g = ws.ensure(want * lane_bytes);
    // HBM shared with other work: halve the request until it fits (at least
    // what the slot held before, or one wave's lanes) instead of failing the call
    while (g == hipErrorOutOfMemory && want > std::max<uint64_t>(64, had)) {
      (void)hipGetLastError();
      want = std::max<uint64_t>(std::max<uint64_t>(64, had), want / 2 / 64 * 64);
      g = ws.ensure(want * lane_bytes);
    }
    return g ? g : more();
  });
}

// The keyed half of a routed enqueue (K14; d.ed_mu[slot] held, the slot's scratch sc
// large enough, s behind the slot's fence): under d.vkey_mu, as every keyed call --
// behind vkeys.ev, followed by vkeys.ev -- the route and partition pass and K12 over
// the keyed list. *routed stays false, and nothing is launched, when no Ed25519 key
// is live any more or the counters cannot be allocated: the caller then takes the
// unrouted path, which is always right. count (K24, the mixed device call; null for the
// dense calls): the device's word with the rows below n to route.
static hipError_t ed_route_and_keyed(Device& d, DevBuf& sc, const uint8_t* keys, const uint8_t* sigs,
                                     const uint8_t* msgs, uint32_t msg_len, uint64_t n, const uint8_t* pre,
                                     uint8_t* status, uint32_t flags, hipStream_t s,
                                     const std::function<hipError_t()>* before_msgs, bool* routed,
                                     const uint32_t* count = nullptr) {
  std::lock_guard<std::mutex> vk(d.vkey_mu);
  if (!d.vkeys.live || !d.vkeys.tab.p) return hipSuccess;
  if (!d.vkeys.route_tot.p) {  // the device's first routed enqueue
    if (d.vkeys.route_tot.ensure(16) != hipSuccess) {
      (void)hipGetLastError();
      return hipSuccess;
    }
    const hipError_t z = hipMemsetAsync(d.vkeys.route_tot.p, 0, 16, s);
    if (z != hipSuccess) return z;
  }
  *routed = true;
  const uint32_t* vtab = d.vkeys.tab.as<uint32_t>();
  return fenced({&d.vkeys.ev}, s, [&] {
    hipError_t e =
        launch_ed25519_route(keys, n, vtab, sc.as<uint32_t>(), d.vkeys.route_tot.as<unsigned long long>(), s, count);
    // the split-prep callers' messages: route and partition needed only the keys
    if (e == hipSuccess && before_msgs) e = (*before_msgs)();
    return e ? e
             : launch_ed25519_verify_keyed_idx(sc.as<uint32_t>(), n, sigs, msgs, msg_len, pre, flags, vtab, status, s);
  });
}

// Enqueue Ed25519 verification of n dense lanes on stream s (device already current).
// With routing on and a live Ed25519 key (K14): route and partition, K12 over the
// keyed list, K1 over the generic list, the verdict words from the statuses -- all on
// s, no count read back. Lock order: ed_mu[slot], then vkey_mu (Device, runtime.hpp);
// vkey_mu is never held while this function waits for a lock, a fence or an allocation.
hipError_t ed_verify_enqueue(Device& d, const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs,
                             uint32_t msg_len, uint64_t n, const uint8_t* pre, uint8_t* status,
                             unsigned long long* verdict, uint32_t flags, hipStream_t s, int slot,
                             const std::function<hipError_t()>* before_msgs) {
  std::lock_guard<std::mutex> g(d.ed_mu[slot]);
  DevBuf& ws = d.ed_ws[slot];
  DevBuf& sc = d.ed_route[slot];
  Fence& ev = d.ed_ev[slot];
  const uint64_t lane_bytes = ed25519_ws_lane_bytes();
  bool want_route = d.route_on.load(std::memory_order_relaxed) && n && n <= ed25519_route_max_lanes();
  if (want_route) {  // a look at the registry; decided for good in ed_route_and_keyed
    std::lock_guard<std::mutex> vk(d.vkey_mu);
    want_route = d.vkeys.live && d.vkeys.tab.p;
  }
  // the scratch grows in powers of two from a floor, like the workspace behind the same
  // fence; no room for it: the batch is verified unrouted
  const size_t sc_bytes = want_route ? ed25519_route_scratch_bytes(n) : 0;
  hipError_t e = ed_ws_grow(d, slot, n, sc.cap < sc_bytes, [&] {
    if (sc.cap < sc_bytes && sc.ensure(sc_bytes) != hipSuccess) {
      (void)hipGetLastError();
      want_route = false;
    }
    return hipSuccess;
  });
  e = e ? e : ev.wait(s);
  bool routed = false;
  if (e == hipSuccess && want_route)
    e = ed_route_and_keyed(d, sc, keys, sigs, msgs, msg_len, n, pre, status, flags, s, before_msgs, &routed);
  if (e == hipSuccess && routed) {
    e = launch_ed25519_verify_idx(keys, sigs, msgs, msg_len, n, d.btab.as<uint32_t>(), pre, status, ws.as<uint32_t>(),
                                  ws.cap / lane_bytes / 64 * 64, flags, sc.as<uint32_t>(), s);
    if (e == hipSuccess && verdict) e = launch_ed25519_status_verdict(status, n, verdict, s);
  } else if (e == hipSuccess) {
    e = launch_ed25519_verify(keys, sigs, msgs, msg_len, n, d.btab.as<uint32_t>(), pre, status, verdict,
                              ws.as<uint32_t>(), ws.cap / lane_bytes / 64 * 64, flags, s, before_msgs);
  }
  if (routed) {  // whatever was launched is fenced, also after a failure
    const hipError_t r = ev.record(s);
    return e ? e : r;
  }
  return e ? e : ev.record(s);
}

// The Ed25519 section of a device signed-tx call (32-byte messages in HBM, on the
// caller's stream s): chunks of CORDAHIP_DEVICE_ED_CHUNK signatures (default
// 98,304 = 0.75 of a ladder round of 2 waves x 1,024 SIMDs x 64 lanes; 0: one
// launch pair) alternate between s with workspace slot 0 and the device's s_ed2
// with slot 1, the short remainder first. Every ladder wave takes about the same
// time, so one launch over C4's 2.5 M signatures (19.07 rounds) ran 20 rounds, its
// last with 7% of the CUs; alternating chunks let chunk k + 1's prep fill chunk k's
// ladder tail, as the host pipelines do. Two streams hold two chunks, so a chunk
// below half a round leaves CUs idle (2^15: C4 64.7 M sig/s). One box
// (profiles/r06_device_ed_chunk_ab/): C4 93.4-94.5 with one launch pair, 95.1-96.4
// at 2^17, 95.8-96.7 at 2^16, 97.0-97.7 at 98,304; C4 --device-encode 87.1-87.2,
// 88.7-89.2, 89.3-89.4, 89.2-89.2.
hipError_t ed_verify_device_chunks(Device& d, TxSet& S, const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs,
                                   uint64_t n, uint8_t* status, hipStream_t s) {
  static const uint64_t chunk = [] {
    const char* v = getenv("CORDAHIP_DEVICE_ED_CHUNK");
    return v ? (uint64_t)strtoull(v, nullptr, 10) / 64 * 64 : (uint64_t)98304;
  }();
  if (!chunk || n <= chunk || !d.s_ed2)
    return ed_verify_enqueue(d, keys, sigs, msgs, 32, n, nullptr, status, nullptr, 0u, s, 0, nullptr);
  hipError_t e = hipEventRecord(S.ed_fork, s);
  e = e ? e : hipStreamWaitEvent(d.s_ed2, S.ed_fork, 0);
  const uint64_t r = n % chunk;
  uint64_t lo = 0;
  for (int k = 0; lo < n && e == hipSuccess; k++) {
    const uint64_t hi = lo + (k == 0 && r ? r : chunk);
    e = ed_verify_enqueue(d, keys + lo * 32, sigs + lo * 64, msgs + lo * 32, 32, hi - lo, nullptr, status + lo,
                          nullptr, 0u, k % 2 ? d.s_ed2 : s, k % 2, nullptr);
    lo = hi;
  }
  e = e ? e : hipEventRecord(S.ed_join, d.s_ed2);
  return e ? e : hipStreamWaitEvent(s, S.ed_join, 0);
}

// K23: a mixed-scheme CSR batch resident in device memory. The packer's three passes
// (sig_pack.hip) leave every class's dense rows and its count in the device's scratch;
// each class's message rows are gathered, its generic engine runs over the rows -- the
// indexed instances, which read the count on the device: Ed25519 over the counter block's
// route-format header with iota as its list, ECDSA over the packer's perm and counters,
// RSA per width class over launch_rsa_pss_verify_counted -- and the rows' statuses go
// back to lane order. One stream, no read-back; the host sizes every launch and every
// buffer for its upper bound (n lanes; an RSA class key_bytes / the smallest key of the
// class).
// K24, cordahip_vkey_set_routing_device on: each family's section follows that family's
// routing switch and live keys, as the dense calls do, through the same helpers
// (ed_route_and_keyed, ec_route_and_keyed, rsa_route_and_keyed) and the counted instances
// of the route passes, which read the class's row count where the packer left it. The
// family's scratch (d.ed_route[0], d.ec[0].route / perm / counters, d.rsa.route) sits
// behind the family's lock and fence, taken here anyway. Lock order: sigpack_mu, the
// family's mutex, vkey_mu; vkey_mu is never held across a wait for a lock, a fence or an
// allocation. No live key, the family's switch off, no room for the scratch: the family
// takes the unrouted launches. Off (the default): the switches are not consulted.
hipError_t sig_device_enqueue(Device& d, const sigpack::In& in, const uint8_t* msgs, uint8_t* status,
                              unsigned long long* verdict, hipStream_t s) {
  using namespace sigpack;
  const uint64_t n = in.n, ml = in.msg_len;
  if (n == 0) return hipSuccess;
  if (n >= kMaxLanes) return hipErrorInvalidValue;
  std::lock_guard<std::mutex> g(d.sigpack_mu);
  SigPackWork& w = d.sigpack;
  const uint64_t nt = tiles(n);
  struct Carve {  // offsets of 256-byte-aligned pieces
    size_t at = 0;
    size_t take(size_t bytes) {
      const size_t o = at;
      at += (bytes + 255) / 256 * 256;
      return o;
    }
  } c, rc;
  const size_t o_hdr = c.take(4 * (kHdrWords + n)), o_code = c.take(n), o_btot = c.take(4 * kCounts * nt),
               o_boff = c.take(4 * kCounts * nt);
  const size_t o_edk = c.take(32 * n), o_eds = c.take(64 * n), o_edp = c.take(n), o_edl = c.take(4 * n),
               o_edm = c.take(4 * n), o_edmsg = c.take(ml * n), o_edst = c.take(n);
  const size_t o_ecsch = c.take(n), o_eck = c.take(65 * n), o_eckl = c.take(n), o_ecs = c.take(72 * n),
               o_ecsl = c.take(n), o_ecp = c.take(n), o_ecl = c.take(4 * n), o_ecm = c.take(4 * n),
               o_ecperm = c.take(4 * n), o_ecmsg = c.take(ml * n), o_ecst = c.take(n);
  uint64_t cap[3] = {0, 0, 0};
  size_t o_rmod[3], o_rexp[3], o_rsig[3], o_rsl[3], o_rpre[3], o_rlane[3], o_rmsg[3], o_rmsgs[3], o_rst[3], o_rlc[3];
  for (uint32_t k = 0; k < 3 && in.rsa_on; k++) {
    const uint64_t r = cap[k] = rsa_cap_rows(kRsa0 + k, n, in.key_bytes), W = rsa_words(kRsa0 + k);
    o_rmod[k] = rc.take(4 * W * r), o_rexp[k] = rc.take(4 * r), o_rsig[k] = rc.take(4 * W * r);
    o_rsl[k] = rc.take(2 * r), o_rpre[k] = rc.take(r), o_rlane[k] = rc.take(4 * r), o_rmsg[k] = rc.take(4 * r);
    o_rmsgs[k] = rc.take(ml * r), o_rst[k] = rc.take(r), o_rlc[k] = rc.take(4 * (r / 64 + 1));
  }
  hipError_t e = w.ev.grow(w.rows.cap < c.at || w.rsa_rows.cap < rc.at, [&] {
    if (w.rows.ensure(c.at) || w.rsa_rows.ensure(rc.at)) return hipErrorOutOfMemory;
    return hipSuccess;
  });
  if (e != hipSuccess) return e;
  e = w.ev.wait(s);
  if (e != hipSuccess) return e;
  uint8_t* base = w.rows.as<uint8_t>();
  uint8_t* rbase = w.rsa_rows.as<uint8_t>();
  const auto at = [](uint8_t* b, size_t o) { return b + o; };
  const auto at32 = [](uint8_t* b, size_t o) { return reinterpret_cast<uint32_t*>(b + o); };
  Out out{};
  out.hdr = at32(base, o_hdr);
  out.code = at(base, o_code);
  out.btot = at32(base, o_btot);
  out.boff = at32(base, o_boff);
  out.status = status;
  out.ed_key = at32(base, o_edk), out.ed_sig = at32(base, o_eds), out.ed_pre = at(base, o_edp);
  out.ed_lane = at32(base, o_edl), out.ed_msg = at32(base, o_edm);
  out.ec_scheme = at(base, o_ecsch), out.ec_key = at(base, o_eck), out.ec_key_len = at(base, o_eckl);
  out.ec_sig = at(base, o_ecs), out.ec_sig_len = at(base, o_ecsl), out.ec_pre = at(base, o_ecp);
  out.ec_lane = at32(base, o_ecl), out.ec_msg = at32(base, o_ecm), out.ec_perm = at32(base, o_ecperm);
  for (uint32_t k = 0; k < 3; k++) {
    out.rsa_cap[k] = cap[k];
    if (!cap[k]) continue;
    out.rsa_mod[k] = at32(rbase, o_rmod[k]), out.rsa_exp[k] = at32(rbase, o_rexp[k]);
    out.rsa_sig[k] = at32(rbase, o_rsig[k]);
    out.rsa_sig_len[k] = reinterpret_cast<uint16_t*>(rbase + o_rsl[k]);
    out.rsa_pre[k] = at(rbase, o_rpre[k]);
    out.rsa_lane[k] = at32(rbase, o_rlane[k]), out.rsa_msg[k] = at32(rbase, o_rmsg[k]);
  }
  const uint32_t* hdr = out.hdr;
  const uint32_t flags = in.do_verify ? 0u : (uint32_t)CORDAHIP_FLAG_IS_VALID;
  const bool dev_route = d.sig_route_on.load(std::memory_order_relaxed) != 0;
  bool launched = false;
  const auto run = [&]() -> hipError_t {
    launched = true;
    hipError_t r = launch_sig_pack(in, out, s);
    if (r != hipSuccess) return r;
    {  // Ed25519: K1's indexed instance over rows 0 .. count; routed (K24): K14's counted
       // partition of those rows, K12 over the keyed list, K1 over the generic list
      uint8_t* em = at(base, o_edmsg);
      uint8_t* est = at(base, o_edst);
      const uint32_t* cnt = hdr + kHdrClass + kEd;
      r = launch_sig_gather(msgs, in.msg_len, out.ed_msg, cnt, n, em, s);
      if (r != hipSuccess) return r;
      std::lock_guard<std::mutex> ge(d.ed_mu[0]);
      DevBuf& sc = d.ed_route[0];
      bool want_route = dev_route && d.route_on.load(std::memory_order_relaxed) && n <= ed25519_route_max_lanes();
      if (want_route) {  // a look at the registry; decided for good in ed_route_and_keyed
        std::lock_guard<std::mutex> vk(d.vkey_mu);
        want_route = d.vkeys.live && d.vkeys.tab.p;
      }
      const size_t sc_bytes = want_route ? ed25519_route_scratch_bytes(n) : 0;
      r = ed_ws_grow(d, 0, n, sc.cap < sc_bytes, [&] {
        if (sc.cap < sc_bytes && sc.ensure(sc_bytes) != hipSuccess) {  // no room: verified unrouted
          (void)hipGetLastError();
          want_route = false;
        }
        return hipSuccess;
      });
      if (r != hipSuccess) return r;
      const uint64_t lane_bytes = ed25519_ws_lane_bytes();
      r = fenced({&d.ed_ev[0]}, s, [&] {
        const uint8_t* ek = reinterpret_cast<const uint8_t*>(out.ed_key);
        const uint8_t* es = reinterpret_cast<const uint8_t*>(out.ed_sig);
        bool routed = false;
        const hipError_t q = want_route ? ed_route_and_keyed(d, sc, ek, es, em, in.msg_len, n, out.ed_pre, est, flags,
                                                             s, nullptr, &routed, cnt)
                                        : hipSuccess;
        if (q != hipSuccess) return q;
        // unrouted: the counter block's route-format header with iota as its list
        return launch_ed25519_verify_idx(ek, es, em, in.msg_len, n, d.btab.as<uint32_t>(), out.ed_pre, est,
                                         d.ed_ws[0].as<uint32_t>(), d.ed_ws[0].cap / lane_bytes / 64 * 64, flags,
                                         routed ? sc.as<uint32_t>() : hdr + kHdrEd, s, routed ? kEdIdxLayoutOfN : 0);
      });
      if (r != hipSuccess) return r;
      r = launch_sig_scatter(est, out.ed_lane, cnt, n, status, s);
      if (r != hipSuccess) return r;
    }
    {  // ECDSA: K2's indexed instance over perm and the engine's counters; routed (K24):
       // K15's seven classes rebuilt over rows 0 .. count in the slot's own perm and
       // counters, K13 over each live curve's run, K2 over the generic list
      uint8_t* cm = at(base, o_ecmsg);
      uint8_t* cst = at(base, o_ecst);
      const uint32_t* cnt = hdr + kHdrClass + kEc;
      r = launch_sig_gather(msgs, in.msg_len, out.ec_msg, cnt, n, cm, s);
      if (r != hipSuccess) return r;
      std::lock_guard<std::mutex> gc(d.ec_mu[0]);
      EcWork& ew = d.ec[0];
      bool want_route = dev_route && d.ec_route_on.load(std::memory_order_relaxed) && n <= ecdsa_route_max_lanes();
      if (want_route) {  // a look at the registry; decided for good in ec_route_and_keyed
        std::lock_guard<std::mutex> vk(d.vkey_mu);
        want_route = d.ec_vkeys.tab.p && d.ec_vkeys.book.any_live();
      }
      const size_t sc_bytes = want_route ? ecdsa_route_scratch_bytes(n) : 0;
      const size_t perm_bytes = want_route ? (size_t)n * 4 : 0;
      const uint64_t slots = std::min<uint64_t>(d.ec_ws_slots, (n + 63) / 64 * 64);
      const bool ws_needed = ew.ws.cap < slots * ecdsa_ws_slot_bytes();
      r = ew.ev.grow(ws_needed || ew.route.cap < sc_bytes || ew.perm.cap < perm_bytes, [&] {
        if (ws_needed) {
          const uint64_t want = std::max<uint64_t>(slots, std::min<uint64_t>(d.ec_ws_slots, kWsMinLanes));
          if (ew.ws.ensure(want * ecdsa_ws_slot_bytes())) return hipErrorOutOfMemory;
        }
        // no room for the route ids or the routed perm: the rows are verified unrouted
        if ((ew.route.cap < sc_bytes && ew.route.ensure(sc_bytes) != hipSuccess) ||
            (ew.perm.cap < perm_bytes && ew.perm.ensure(perm_bytes) != hipSuccess)) {
          (void)hipGetLastError();
          want_route = false;
        }
        return hipSuccess;
      });
      if (r != hipSuccess) return r;
      if (want_route && ew.counters.ensure(64) != hipSuccess) {
        (void)hipGetLastError();
        want_route = false;
      }
      r = fenced({&ew.ev}, s, [&] {
        bool routed = false;
        const hipError_t q =
            want_route ? ec_route_and_keyed(d, ew, out.ec_scheme, out.ec_key, out.ec_key_len, out.ec_sig,
                                            out.ec_sig_len, cm, nullptr, in.msg_len, n, out.ec_pre, cst, flags, s,
                                            &routed, cnt)
                       : hipSuccess;
        if (q != hipSuccess) return q;
        // unrouted: the packer's perm and the counters it left in the engine's format
        return launch_ecdsa_verify_routed(out.ec_scheme, out.ec_key, out.ec_key_len, out.ec_sig, out.ec_sig_len, cm,
                                          nullptr, in.msg_len, n, d.gtab_k1.as<uint32_t>(), d.gtab_r1.as<uint32_t>(),
                                          out.ec_pre, cst, nullptr,
                                          routed ? ew.counters.as<unsigned int>() : hdr + kHdrEc,
                                          routed ? ew.perm.as<unsigned int>() : out.ec_perm, ew.ws.as<uint32_t>(),
                                          ew.ws.cap / ecdsa_ws_slot_bytes() / 64 * 64, flags, s);
      });
      if (r != hipSuccess) return r;
      r = launch_sig_scatter(cst, out.ec_lane, cnt, n, status, s);
      if (r != hipSuccess) return r;
    }
    for (uint32_t k = 0; k < 3; k++) {  // RSA: one width class per launch set
      if (!cap[k]) continue;
      const uint32_t W = rsa_words(kRsa0 + k);
      const uint32_t* cnt = hdr + kHdrClass + kRsa0 + k;
      uint8_t* rm = at(rbase, o_rmsgs[k]);
      uint8_t* rst = at(rbase, o_rst[k]);
      r = launch_sig_gather(msgs, in.msg_len, out.rsa_msg[k], cnt, cap[k], rm, s);
      if (r != hipSuccess) return r;
      std::lock_guard<std::mutex> gr(d.rsa_mu);
      RsaWork& rw = d.rsa;
      r = rsa_ws_grow(d, W, cap[k]);
      if (r != hipSuccess) return r;
      bool want_route = dev_route && d.rsa_route_on.load(std::memory_order_relaxed);
      if (want_route) {  // a look at the registry; decided for good, per launch, in rsa_route_and_keyed
        std::lock_guard<std::mutex> vk(d.vkey_mu);
        want_route = d.rsa_vkeys.live && d.rsa_vkeys.tab.p;
      }
      const uint64_t ws_rows = rsa_ws_rows(rw, W), lr = rsa_launch_rows(ws_rows);
      const uint64_t cap_rows = std::min<uint64_t>(lr, (cap[k] + 63) / 64 * 64);
      want_route = want_route && lr;
      const size_t sc_bytes = want_route ? rsa_route_scratch_bytes(cap_rows) : 0;
      r = rw.ev.grow(rw.route.cap < sc_bytes, [&] {
        if (rw.route.ensure(sc_bytes) != hipSuccess) {  // no room: the class is verified unrouted
          (void)hipGetLastError();
          want_route = false;
        }
        return hipSuccess;
      });
      if (r != hipSuccess) return r;
      const uint8_t* rsig = reinterpret_cast<const uint8_t*>(out.rsa_sig[k]);
      unsigned int* rlc = at32(rbase, o_rlc[k]);
      r = fenced({&rw.ev}, s, [&]() -> hipError_t {
        if (!want_route)
          return launch_rsa_pss_verify_counted(out.rsa_mod[k], out.rsa_exp[k], rsig, out.rsa_sig_len[k], rm,
                                               in.msg_len, W, cap[k], cnt, hdr + kHdrWords, rlc, rst,
                                               rw.ws.as<uint8_t>(), ws_rows, flags, s);
        // K20's head / keyed / tail per launch of the workspace loop, each launch's rows
        // clipped on the device (K23's convention: launch j's in rlc[j])
        hipError_t q = hipSuccess;
        uint64_t j = 0;
        for (uint64_t lo = 0; lo < cap[k] && q == hipSuccess; lo += lr, j++) {
          const uint64_t m = std::min(lr, cap[k] - lo);
          q = launch_rsa_routed_head(out.rsa_mod[k], out.rsa_exp[k], rsig, out.rsa_sig_len[k], nullptr, in.msg_len, W,
                                     lo, m, nullptr, rw.ws.as<uint8_t>(), ws_rows, flags, s, cnt, rlc + j);
          bool routed = false;
          q = q ? q
                : rsa_route_and_keyed(d, out.rsa_mod[k], out.rsa_exp[k], W, lo, m, ws_rows, cap_rows, s, &routed,
                                      rlc + j);
          q = q ? q
                : launch_rsa_routed_tail(out.rsa_mod[k], out.rsa_exp[k], rm, nullptr, in.msg_len, W, lo, m, rst,
                                         nullptr, rw.ws.as<uint8_t>(), ws_rows, rw.route.as<uint32_t>(), cap_rows,
                                         routed, s, rlc + j, hdr + kHdrWords);
        }
        return q;
      });
      if (r != hipSuccess) return r;
      r = launch_sig_scatter(rst, out.rsa_lane[k], cnt, cap[k], status, s);
      if (r != hipSuccess) return r;
    }
    return verdict ? launch_ed25519_status_verdict(status, n, verdict, s) : hipSuccess;
  };
  e = run();
  if (launched) {  // whatever was launched is fenced, also after a failure
    const hipError_t r = w.ev.record(s);
    return e ? e : r;
  }
  return e;
}

// CORDAHIP_DEVICE_MEM_BUDGET (bytes, K/M/G suffixes; default 128 GiB, at most 90%
// of the device): the workspaces it sizes -- Ed25519 slot 0 45% of it, slot 1 20%
// (and half of slot 0 at most), ECDSA 15% -- each also capped by its r05 maximum
// (2^24 lanes / slots, CORDAHIP_ED25519_WS_LANES / CORDAHIP_ECDSA_WS_SLOTS). The
// default therefore keeps C2's single 2^24-lane launch pair (40.8 GB) and the
// r05 lane counts: 40.8 + 20.4 + 18.8 GB of workspaces. The other buffers follow the
// batches (the id and signature stages, component slices, C5's stages) and are
// not split. A smaller budget costs extra launch pairs, never a failed batch.
uint64_t parse_bytes(const char* v, uint64_t dflt) {
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const double x = strtod(v, &end);
  if (end == v || x <= 0) return dflt;
  const char u = end ? (char)toupper((unsigned char)*end) : 0;
  const double m = u == 'K' ? 1024.0 : u == 'M' ? 1048576.0 : u == 'G' ? 1073741824.0 : 1.0;
  return (uint64_t)(x * m);
}

void device_budget(Device& d) {  // device current
  uint64_t b = parse_bytes(getenv("CORDAHIP_DEVICE_MEM_BUDGET"), 128ull << 30);
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot) b = std::min<uint64_t>(b, (uint64_t)tot / 10 * 9);
  d.mem_budget = b;
  auto lanes = [](uint64_t bytes, uint64_t per) { return std::max<uint64_t>(64, bytes / per / 64 * 64); };
  const uint64_t lb = ed25519_ws_lane_bytes(), sb = ecdsa_ws_slot_bytes();
  d.ed_ws_lanes[0] = std::min(env_lanes("CORDAHIP_ED25519_WS_LANES", kEdWsLanes), lanes(b / 100 * 45, lb));
  d.ed_ws_lanes[1] = std::min(std::max<uint64_t>(64, d.ed_ws_lanes[0] / 2 / 64 * 64), lanes(b / 5, lb));
  d.ec_ws_slots = std::min(env_lanes("CORDAHIP_ECDSA_WS_SLOTS", kEcWsSlots), lanes(b / 100 * 15, sb));
}

// Free an idle device's grow-only buffers (the idle release, cordahip_trim): both
// buffer sets and every lock that guards a buffer, in an order every path keeps;
// Device::release_idle then waits for the fences of the device-path users (kernels
// on caller streams) and frees what it does not keep (the fixed tables, the
// encoder's shape table and the ECDSA counters stay: derived data, 18 MB).
void trim_device(Device& d) {
  SetLease l0(d, 0, true), l1(d, 1, true);
  std::lock_guard<std::mutex> gk(d.kryo_mu), gs(d.stream_mu), gp(d.ped_mu), gsp(d.sigpack_mu), ge0(d.ed_mu[0]),
      ge1(d.ed_mu[1]),
      gc0(d.ec_mu[0]), gc1(d.ec_mu[1]), gr(d.rsa_mu), gv(d.cover_mu), gh(d.sign_stage.mu), gvh(d.vkey_stage.mu);
  if (hipSetDevice(d.id) != hipSuccess) return;
  d.release_idle();
  if (tracing()) fprintf(stderr, "[cordahip] dev %d: idle buffers released\n", d.id);
}

void secure_wipe(void* p, size_t n) {
  volatile unsigned char* v = static_cast<volatile unsigned char*>(p);
  while (n--) *v++ = 0;
}

// The signer's key records zeroed on every device: after every signing kernel
// that may read them (keys.ev), before ~Device frees the tables.
void signer_wipe(cordahip_ctx* ctx) {
  for (auto& dp : ctx->devs) {
    Device& d = *dp;
    std::lock_guard<std::mutex> g(d.sign_mu);
    bool any = false;
    d.signer_keys([&](auto& k) {  // each family's secret bytes (KeyTable), behind its fence
      if (!k.tab.p || hipSetDevice(d.id) != hipSuccess) return;
      any = true;
      (void)k.ev.sync();
      const TabSpan z = k.secrets();
      (void)hipMemsetAsync(k.tab.template as<uint8_t>() + z.at, 0, z.bytes, d.stream);
    });
    if (any) (void)hipStreamSynchronize(d.stream);
  }
}

// the in-process partition rule (cordahip_shard_range)
void shard_range(uint64_t n, uint64_t nshards, uint64_t shard, uint64_t align, uint64_t& lo, uint64_t& hi) {
  if (nshards == 0 || shard >= nshards) {
    lo = hi = n;
    return;
  }
  align = align ? align : 1;
  const uint64_t per = ((n + nshards - 1) / nshards + align - 1) / align * align;
  lo = std::min(n, shard * per);
  hi = std::min(n, lo + per);
}

}  // namespace rt
}  // namespace cordahip

static std::atomic<uint64_t> g_device_uid{1};

extern "C" {

static int init_impl(uint32_t device_mask, cordahip_ctx** out) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return CORDAHIP_ERR_NO_DEVICE;
  auto ctx = std::make_unique<cordahip_ctx>();
  int rc = CORDAHIP_SUCCESS;
  // Test-only: CORDAHIP_TEST_DEVICE_REPLICAS=k gives the context k Device
  // objects per selected HIP device (each with its own streams, buffers and
  // tables), so the N-device code -- shard split, per-device workers, tails,
  // verdict reassembly -- runs on a one-GPU box. Unset in production.
  int replicas = 1;
  if (const char* v = getenv("CORDAHIP_TEST_DEVICE_REPLICAS")) replicas = std::max(1, std::min(8, atoi(v)));
  std::vector<int> ids;
  for (int d = 0; d < count && d < kMaxHipDevices; d++)
    if (!device_mask || ((device_mask >> d) & 1u))
      for (int r = 0; r < replicas; r++) ids.push_back(d);
  for (int d : ids) {
    if (rc != CORDAHIP_SUCCESS) break;
    ctx->devs.push_back(std::make_unique<Device>());
    Device& dev = *ctx->devs.back();
    dev.bind(d);
    dev.uid = g_device_uid.fetch_add(1);
    if (hipSetDevice(d) != hipSuccess || hipStreamCreateWithFlags(&dev.stream, hipStreamNonBlocking) != hipSuccess) {
      rc = CORDAHIP_ERR_HIP;
      break;
    }
    for (TxSet& S : dev.set)
      for (hipEvent_t* pe : {&S.fork, &S.ids, &S.ed_fork, &S.ed_join})
        if (hipEventCreateWithFlags(pe, hipEventDisableTiming) != hipSuccess) rc = CORDAHIP_ERR_HIP;
    if (rc != CORDAHIP_SUCCESS) break;
    for (auto& tc : dev.ring)
      if (hipEventCreate(&tc.a) != hipSuccess || hipEventCreate(&tc.b) != hipSuccess) rc = CORDAHIP_ERR_HIP;
    if (rc != CORDAHIP_SUCCESS) break;
    if (dev.btab.ensure(ed25519_btable_bytes() + ed25519_comb_bytes()) || dev.gtab_k1.ensure(ecdsa_gtable_bytes()) ||
        dev.gtab_r1.ensure(ecdsa_gtable_bytes())) {
      rc = CORDAHIP_ERR_OUT_OF_MEMORY;
      break;
    }
    device_budget(dev);
    static const bool id_prio = !(getenv("CORDAHIP_ID_PRIO") && getenv("CORDAHIP_ID_PRIO")[0] == '0');
    if (!id_prio && (tx_set_id_priority(0) != hipSuccess || kryo_set_priority(0) != hipSuccess)) {
      rc = CORDAHIP_ERR_HIP;
      break;
    }
    if (launch_ed25519_btable(dev.btab.as<uint32_t>(), dev.stream) != hipSuccess ||
        launch_ed25519_comb(dev.comb(), dev.stream) != hipSuccess ||
        launch_ecdsa_gtables(dev.gtab_k1.as<uint32_t>(), dev.gtab_r1.as<uint32_t>(), dev.stream) != hipSuccess ||
        hipStreamSynchronize(dev.stream) != hipSuccess)
      rc = CORDAHIP_ERR_HIP;
  }
  if (rc == CORDAHIP_SUCCESS && ctx->devs.empty()) rc = CORDAHIP_ERR_NO_DEVICE;
  if (rc != CORDAHIP_SUCCESS) return rc;  // ~Device frees what the devices got
  ctx->pool = std::make_unique<WorkerPool>((int)std::max<size_t>(2, 2 * ctx->devs.size()));
  // host threads. Per device (numa_place.hpp): a pool bound to CPUs of the GPU's
  // NUMA node -- the devices of one node split its CPUs -- of CORDAHIP_HOST_THREADS
  // threads at most (default 16: the pipelines are PCIe / kernel bound beyond that,
  // tools/pack_bench.cpp); CORDAHIP_NUMA=0 leaves them unbound. Context-wide: a
  // pool for the batch-level passes (CSR checks, verdict words) of at most 16.
  int cap = 16;
  if (const char* v = getenv("CORDAHIP_HOST_THREADS")) cap = std::max(1, std::min(256, atoi(v)));
  std::vector<int> allowed;
  {
    cpu_set_t cs;
    if (sched_getaffinity(0, sizeof(cs), &cs) == 0)
      for (int c = 0; c < CPU_SETSIZE; c++)
        if (CPU_ISSET(c, &cs)) allowed.push_back(c);
  }
  if (allowed.empty())
    for (int c = 0; c < (int)std::max(1u, std::thread::hardware_concurrency()); c++) allowed.push_back(c);
  std::vector<std::string> pci(ctx->devs.size());
  const bool numa = !(getenv("CORDAHIP_NUMA") && getenv("CORDAHIP_NUMA")[0] == '0');
  for (size_t i = 0; i < ctx->devs.size() && numa; i++) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, ctx->devs[i]->id) == hipSuccess) {
      pci[i] = bus;
      for (char& ch : pci[i]) ch = (char)tolower((unsigned char)ch);
    }
  }
  const char* root = getenv("CORDAHIP_SYSFS_ROOT");  // tests: a fake tree
  const std::vector<NumaPlace> plan = numa_plan(root ? root : "/sys", pci, allowed, cap);
  for (size_t i = 0; i < ctx->devs.size(); i++) {
    Device& d = *ctx->devs[i];
    d.place = plan[i];
    if (!numa) d.place.cpus.clear();
    d.pool = std::make_unique<HostPool>(d.place.threads, d.place.cpus);
    if (tracing())
      fprintf(stderr, "[cordahip] dev %d (%s): NUMA node %d, %zu CPUs, %d host threads%s%s\n", d.id, pci[i].c_str(),
              d.place.node, d.place.cpus.size(), d.place.threads, d.place.why.empty() ? "" : ": ",
              d.place.why.c_str());
  }
  ctx->host = std::make_unique<HostPool>(std::max(1, std::min<int>((int)allowed.size(), 16)));
  // the idle release: a device with no call for CORDAHIP_IDLE_RELEASE_MS (default 30 s;
  // 0: never) gives its grow-only buffers back (trim_device)
  const char* iv = getenv("CORDAHIP_IDLE_RELEASE_MS");
  const int64_t idle_ms = iv ? strtoll(iv, nullptr, 10) : 30000;
  if (idle_ms > 0) {
    cordahip_ctx* c = ctx.get();
    c->reaper = std::thread([c, idle_ms] {
      std::vector<int64_t> trimmed_at(c->devs.size(), 0);  // the last call's end when last trimmed
      std::unique_lock<std::mutex> g(c->reaper_mu);
      while (!c->reaper_stop) {
        c->reaper_cv.wait_for(g, std::chrono::milliseconds(std::min<int64_t>(250, idle_ms)));
        if (c->reaper_stop) break;
        for (size_t i = 0; i < c->devs.size(); i++) {
          Device& d = *c->devs[i];
          const int64_t last = d.last_use_ms.load();
          if (d.active.load() > 0 || last == 0 || last == trimmed_at[i] || (int64_t)now_ms() - last < idle_ms)
            continue;
          g.unlock();
          trim_device(d);
          g.lock();
          trimmed_at[i] = last;
        }
      }
    });
  }
  *out = ctx.release();
  return CORDAHIP_SUCCESS;
}

int cordahip_init(uint32_t device_mask, cordahip_ctx** out) {
  if (!out) return CORDAHIP_ERR_INVALID_ARG;
  *out = nullptr;
  return guarded([&] { return init_impl(device_mask, out); });
}

void cordahip_shutdown(cordahip_ctx* ctx) {
  if (!ctx) return;
  if (ctx->reaper.joinable()) {
    {
      std::lock_guard<std::mutex> g(ctx->reaper_mu);
      ctx->reaper_stop = true;
    }
    ctx->reaper_cv.notify_all();
    ctx->reaper.join();
  }
  ctx->pool.reset();  // runs every queued job to completion, joins the workers
  ctx->host.reset();
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    ctx->jobs.clear();
  }
  signer_wipe(ctx);  // no key record outlives the context in device memory
  delete ctx;  // ~Device frees each device's buffers, events and streams
}

}  // extern "C"
