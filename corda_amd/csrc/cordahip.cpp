// libcordahip.so host runtime: contexts, devices, streams, pinned memory,
// batch partitioning and the C-ABI of include/cordahip.h.
//
// MI355X-first shape: one context drives the devices named by its mask; a
// host batch is split into contiguous 64-aligned shards, one per device
// (Ed25519 and ECDSA lanes alike; transactions whole), and each shard streams
// through HIP streams in fixed chunks (H2D of chunk k+1 overlaps the kernel of
// chunk k). Device buffers are grow-only per device and reused across calls;
// every buffer shared between streams is fenced by an event (the next user's
// stream waits on the last user's completion). Tickets run on a per-context
// worker pool. The fixed-base tables are built once per device at init by a
// kernel. There is no CPU verification fallback: a HIP failure is returned to
// the caller as CORDAHIP_ERR_HIP. The generic CSR signature batch lives in
// host_batch.cpp; the registered-key calls in keyed.cpp; the notary commit log in
// commit_api.cpp; the shared runtime types in runtime.hpp; the per-device runtime
// (pools, streams, budget, enqueue helpers, idle release, init / shutdown) in
// runtime.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_support.hpp"
#include "cover_core.hpp"
#include "csr_check.hpp"
#include "notary_stage.hpp"
#include "kryo_core.hpp"
#include "runtime.hpp"
#include "sig_pack.hpp"
#include "status.hpp"

using namespace cordahip;
using namespace cordahip::rt;

// device uid -> (ring slot, generation) of this thread's most recent timed call
static thread_local std::unordered_map<uint64_t, std::pair<int, uint64_t>> tl_last_call;

uint64_t cordahip::rt::submit_job(cordahip_ctx* ctx, std::function<int()> fn) {
  auto st = std::make_shared<JobState>();
  uint64_t t;
  {
    std::lock_guard<std::mutex> g(ctx->mu);
    t = ctx->next_ticket++;
    ctx->jobs.emplace(t, st);
  }
  ctx->pool->push(st, std::move(fn));
  return t;
}

// timing slot for one *_device call (records `a` now on stream s); the slot's
// generation is the call's sequence number, so a reader whose slot was reused
// by a later call (more than kTimingRing calls in between) can tell
TimedCall* cordahip::rt::timed_begin(Device& d, hipStream_t s) {
  std::lock_guard<std::mutex> g(d.tmu);
  const uint64_t seq = ++d.ring_next;
  const int idx = (int)(seq % kTimingRing);
  TimedCall* tc = &d.ring[idx];
  tc->gen = seq;
  if (hipEventRecord(tc->a, s) != hipSuccess) return nullptr;
  tl_last_call[d.uid] = {idx, seq};
  return tc;
}

namespace {

// a zeroed 64-byte host-mapped buffer (the encoder's usage reports)
hipError_t usage_buffer(PinBuf& h, uint32_t*& dp) {
  if (h.p) return hipSuccess;
  void* dv = nullptr;
  if (h.ensure(64, hipHostMallocMapped) != hipSuccess) return hipErrorOutOfMemory;
  if (hipHostGetDevicePointer(&dv, h.p, 0) != hipSuccess) {
    h.release();
    return hipErrorUnknown;
  }
  std::memset(h.p, 0, 64);
  dp = static_cast<uint32_t*>(dv);
  return hipSuccess;
}

// The Kryo encoder's persistent state ready for a call on stream s (kryo_mu
// held, d.kryo_fixed allocated): zeroed when freshly allocated; cleared when the
// usage a call reported passes half the table or nearly fills the template
// arena (recurring shapes then rebuild once). The reports are snapshots of
// counters that only grow between clears, so the largest one is the latest; a
// report may lag by the calls still running (cordahip_kryo_encode_device's is
// read without waiting for its stream): the table then clears one call later,
// and until then new shapes take the direct encoder -- slower, never wrong.
hipError_t kryo_state_ready(Device& d, hipStream_t s) {
  if (hipError_t e = usage_buffer(d.kryo_usage, d.kryo_usage_dev)) return e;
  uint32_t templates = 0, slots = 0;
  for (const PinBuf* b : {&d.kryo_usage, &d.set[0].kryo_usage, &d.set[1].kryo_usage})
    if (b->p) {
      const volatile uint32_t* u = b->as<uint32_t>();
      templates = std::max<uint32_t>(templates, (uint32_t)u[0]);
      slots = std::max<uint32_t>(slots, (uint32_t)u[1]);
    }
  if (d.kryo_fresh || templates > kryo_clear_threshold_templates() || slots > kryo_clear_threshold_slots()) {
    d.kryo_fresh = false;
    d.kryo_templates_ok = false;  // an empty table: the next component batch builds its shapes
    d.kryo_gen++;                 // a call that started before the clear does not vouch for the new table
    for (const PinBuf* b : {&d.kryo_usage, &d.set[0].kryo_usage, &d.set[1].kryo_usage})
      if (uint32_t* p = b->as<uint32_t>()) p[0] = p[1] = 0;
    return kryo_clear(d.kryo_fixed.as<uint8_t>(), s);
  }
  return hipSuccess;
}
// after a call's encoder launches: its usage counters to the host-mapped copy of
// its set (nullptr: cordahip_kryo_encode_device's own)
hipError_t kryo_usage_report(Device& d, TxSet* set, hipStream_t s) {
  return launch_store_to_host(kryo_usage_src(d.kryo_fixed.as<uint8_t>()),
                              set ? set->kryo_usage_dev : d.kryo_usage_dev, kKryoUsageBytes, s);
}
// The encoder's scratch for n items (kryo_mu held, device current): leaf sizes, item
// slots, the direct writers' level buffers, the fixed part (once: its size is fixed;
// marked fresh) and, for the calls that write leaves, temp_bytes of scan storage
// (0: left as it is). kryo_ev fences all of it.
constexpr uint64_t kKryoDirectWriters = 1u << 13;  // 2^13 threads, 7 KB of level buffers each (56 MB)
hipError_t kryo_scratch_ensure(Device& d, uint64_t n, size_t temp_bytes) {
  const size_t ws = kryo_direct_ws_bytes(kKryoDirectWriters), fixed = kryo_fixed_scratch_bytes();
  const bool grow = d.kryo_sizes.cap < (n + 1) * 8 || d.kryo_temp.cap < temp_bytes || d.kryo_items.cap < n * 8 + 8 ||
                    d.kryo_ws.cap < ws || d.kryo_fixed.cap < fixed;
  return d.kryo_ev.grow(grow, [&] {
    if (d.kryo_fixed.cap < fixed) d.kryo_fresh = true;
    return d.kryo_sizes.ensure((n + 1) * 8) || d.kryo_temp.ensure(temp_bytes) ||
                   d.kryo_items.ensure(n * 8 + 8) || d.kryo_ws.ensure(ws) || d.kryo_fixed.ensure(fixed)
               ? hipErrorOutOfMemory
               : hipSuccess;
  });
}

// What the two device signed-tx entry points share (leaves or components in HBM,
// Ed25519 signatures, everything on the caller's stream s): the set's buffers, the
// fork of the id chain, and -- once the caller has enqueued its id chain on x -- the
// signatures over the ids and the per-transaction reduce.
// CORDAHIP_DEVICE_SPLIT=1: the id chain forks onto the device's id stream and runs
// beside the key half of the Ed25519 prep (key and R decoding: no dependence on the
// ids) on s, which joins it before the message half. Off by default: the split prep's
// two launches cost more than the overlap gains (c4 --device-encode 87.3-87.4 against
// 89.1-89.2 M sig/s, c4 95.6-95.9 against 96.1-96.5; profiles/r06_device_split_ab/).
struct DeviceSignedTx {
  Device& d;
  TxSet& S;
  uint64_t ntx;
  const void *d_tx_sig_off, *d_keys, *d_sigs;
  uint64_t nsig;
  void *d_txid, *d_tx_status, *d_first_bad, *d_sig_status;
  // K23, the mixed-scheme forms: the signatures as a CSR batch with a scheme byte each
  // (d_keys / d_sigs unused); its message rows are the ids, indexed by transaction
  const sigpack::In* mixed = nullptr;
  static bool split() {
    static const bool on = getenv("CORDAHIP_DEVICE_SPLIT") && getenv("CORDAHIP_DEVICE_SPLIT")[0] == '1';
    return on;
  }
  // the set's leaf hashes and message rows (component calls: their statuses too), the streams
  hipError_t prepare(uint64_t nleaves, bool comp_status) const {
    TxWork& w = S.tx;
    const uint64_t hb = std::max<uint64_t>(nleaves, 1) * 32, mb = std::max<uint64_t>(nsig, 1) * 32,
                   cb = comp_status ? std::max<uint64_t>(nleaves, 1) : 0;
    const hipError_t e = S.tx_ev.grow(w.hashes.cap < hb || w.msgs.cap < mb || w.comp_status.cap < cb, [&] {
      return w.hashes.ensure(hb) || w.msgs.ensure(mb) || w.comp_status.ensure(cb) ? hipErrorOutOfMemory : hipSuccess;
    });
    return e ? e : ensure_streams(d);
  }
  // s waits for the set's previous user; x: the stream of the id chain
  hipError_t fork(hipStream_t s, hipStream_t& x) const {
    x = split() ? d.s_idcopy : s;
    hipError_t e = S.tx_ev.wait(s);
    if (split()) {
      e = e ? e : hipEventRecord(S.fork, s);
      e = e ? e : hipStreamWaitEvent(x, S.fork, 0);
    }
    return e;
  }
  hipError_t join_and_verify(hipStream_t s, hipStream_t x) const {
    TxWork& w = S.tx;
    const uint8_t *keys = static_cast<const uint8_t*>(d_keys), *sigs = static_cast<const uint8_t*>(d_sigs);
    uint8_t* sig_status = static_cast<uint8_t*>(d_sig_status);
    hipError_t e = split() ? hipEventRecord(S.ids, x) : hipSuccess;
    if (mixed) {
      // the ids first; every signature's message row is its transaction's index (the set's
      // message buffer holds the indices: nothing is gathered per signature here), then the
      // packer and the three families' generic verifiers (runtime.cpp sig_device_enqueue)
      if (split()) e = e ? e : hipStreamWaitEvent(s, S.ids, 0);
      sigpack::In in = *mixed;
      in.msg_row = w.msgs.as<uint32_t>();
      in.msg_rows = ntx;
      in.msg_len = 32;
      e = e ? e : launch_sig_tx_rows(static_cast<const uint64_t*>(d_tx_sig_off), ntx, nsig, w.msgs.as<uint32_t>(), s);
      e = e ? e : sig_device_enqueue(d, in, static_cast<const uint8_t*>(d_txid), sig_status, nullptr, s);
      e = e ? e : S.tx_ev.record(s);
      return e ? e : launch_tx_reduce(sig_status, static_cast<const uint64_t*>(d_tx_sig_off), ntx,
                                      static_cast<int64_t*>(d_first_bad), static_cast<uint8_t*>(d_tx_status), s);
    }
    const std::function<hipError_t()> join = [&]() -> hipError_t {  // the ids, then the signatures' messages
      hipError_t r = split() ? hipStreamWaitEvent(s, S.ids, 0) : hipSuccess;
      return r ? r : launch_gather_txid(static_cast<const uint8_t*>(d_txid), static_cast<const uint64_t*>(d_tx_sig_off),
                                        ntx, w.msgs.as<uint8_t>(), s);
    };
    // unforked, the ids come first and the prep runs fused (its key and message halves
    // as two launches cost ~0.6 ms more per 2.5 M signatures with nothing beside them)
    if (nsig == 0 || !split()) e = e ? e : join();
    if (split())
      e = e ? e : ed_verify_enqueue(d, keys, sigs, w.msgs.as<uint8_t>(), 32, nsig, nullptr, sig_status, nullptr, 0u, s,
                                    0, nsig ? &join : nullptr);
    else
      e = e ? e : ed_verify_device_chunks(d, S, keys, sigs, w.msgs.as<uint8_t>(), nsig, sig_status, s);
    e = e ? e : S.tx_ev.record(s);  // fences the set's buffers for the next user
    return e ? e : launch_tx_reduce(sig_status, static_cast<const uint64_t*>(d_tx_sig_off), ntx,
                                    static_cast<int64_t*>(d_first_bad), static_cast<uint8_t*>(d_tx_status), s);
  }
};

// A leased set's buffers for a host tx path: the last device-path user of the
// set may still be running kernels on its own stream.
int tx_acquire_host(Device& d, TxSet& set) {
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  if (set.tx_ev.sync() != hipSuccess) return CORDAHIP_ERR_HIP;
  return CORDAHIP_SUCCESS;
}

// Transaction ids for txs [t0, t1) on one device. The caller's offset arrays go
// to the device as they are (absolute offsets, no host rebasing pass): the
// kernels get base pointers shifted by the shard's first byte / first leaf.
int tx_ids_shard(cordahip_ctx* ctx, Device& d, const cordahip_txid_batch* b, uint64_t t0, uint64_t t1) {
  (void)ctx;
  SetLease lease(d);
  TxSet& S = lease.get();
  const NodeBind nb(d);
  const Activity act(d);
  if (int rc = tx_acquire_host(d, S)) return rc;
  const uint64_t ntx = t1 - t0;
  const uint64_t l0 = b->tx_leaf_off[t0], l1 = b->tx_leaf_off[t1];
  const uint64_t nleaves = l1 - l0;
  const uint64_t b0 = b->leaf_off[l0], b1 = b->leaf_off[l1];
  TxWork& w = S.tx;
  if (w.leaf_bytes.ensure(std::max<uint64_t>(b1 - b0, 16)) || w.leaf_off.ensure((nleaves + 1) * 8) ||
      w.tx_leaf_off.ensure((ntx + 1) * 8) || w.hashes.ensure(std::max<uint64_t>(nleaves, 1) * 32) ||
      w.txid.ensure(ntx * 32) || w.tx_status.ensure(ntx))
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  hipStream_t s = d.stream;
  hipError_t e = hipSuccess;
  if (b1 > b0) e = hipMemcpyAsync(w.leaf_bytes.p, b->leaf_bytes + b0, b1 - b0, hipMemcpyHostToDevice, s);
  e = e ? e : hipMemcpyAsync(w.leaf_off.p, b->leaf_off + l0, (nleaves + 1) * 8, hipMemcpyHostToDevice, s);
  e = e ? e : hipMemcpyAsync(w.tx_leaf_off.p, b->tx_leaf_off + t0, (ntx + 1) * 8, hipMemcpyHostToDevice, s);
  // leaf i's bytes at leaf_bytes + (leaf_off[l0 + i] - b0); tx t's hashes at hashes + (tx_leaf_off[t] - l0) * 8
  const uint8_t* bytes_base = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(w.leaf_bytes.p) - b0);
  uint32_t* hash_base = reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(w.hashes.p) - l0 * 32);
  e = e ? e : launch_sha256_leaves(bytes_base, w.leaf_off.as<uint64_t>(), nleaves, w.hashes.as<uint32_t>(), s);
  e = e ? e : launch_merkle_root(hash_base, w.tx_leaf_off.as<uint64_t>(), ntx, w.txid.as<uint8_t>(),
                                 w.tx_status.as<uint8_t>(), s);
  e = e ? e : hipMemcpyAsync(b->txid + t0 * 32, w.txid.p, ntx * 32, hipMemcpyDeviceToHost, s);
  e = e ? e : hipMemcpyAsync(b->tx_status + t0, w.tx_status.p, ntx, hipMemcpyDeviceToHost, s);
  e = e ? e : S.tx_ev.record(s);
  e = e ? e : S.tx_ev.sync();
  if (e != hipSuccess) (void)hipStreamSynchronize(s);
  return hip_err(e);
}

int tx_ids_impl(cordahip_ctx* ctx, const cordahip_txid_batch* b) {
  if (b->ntx && (!b->leaf_off || !b->tx_leaf_off || !b->txid || !b->tx_status || !b->leaf_bytes))
    return CORDAHIP_ERR_INVALID_ARG;
  if (b->ntx == 0) return CORDAHIP_SUCCESS;
  if (!check_txid_batch(PoolPar{*ctx->host}, b)) return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  // contiguous tx shards: a transaction's tree stays on one device
  return for_shards(ctx->devs, b->ntx, 1,
                    [&](Device& d, uint64_t t0, uint64_t t1) { return tx_ids_shard(ctx, d, b, t0, t1); });
}

// The tx ids of one device's shard, in slices on the device's context stream
// (the set S leased, its previous users finished): slice j's leaf bytes and
// offsets go H2D into their region of whole-shard buffers (offset arrays
// unchanged, shifted base pointers) on d.s_idcopy, followed by cev[j]; its
// SHA-256 and Merkle kernels run on the context stream behind cev[j], then
// kev[j] marks its ids in HBM, its ids and statuses come back, and ev[j] marks
// them on the host. tx_ids_prepare sizes the buffers once; tx_ids_enqueue
// enqueues slices [j0, j1) (the signed-tx path releases them a few at a time,
// interleaved with the signature chunks' copies, because H2D copies of all
// streams leave through the DMA engine in submission order).
// Leaf bytes one component may need (kryo_core.hpp): the kind's constant text
// (class and field names, framing; < 2 KB for a cash state) plus at most 4
// bytes per payload byte (a cash state writes the owner's key and name up to 3
// times; a string 3 bytes per UTF-16 unit). A leaf beyond its slice's bound
// would be reported, not written (CORDAHIP_TX_BAD_COMPONENT);
// tests/test_kryo_template.py checks the bound on every test item.
uint64_t comp_leaf_bound(uint64_t payload_bytes) { return 4096 + 4 * payload_bytes; }
uint64_t comp_payload_bytes(const cordahip_kryo_item& it) {
  return (it.kind == CORDAHIP_KRYO_STRING || it.kind == CORDAHIP_KRYO_KOTLIN_OBJECT) ? 2 * it.len : it.len;
}

// Component-level batches (cordahip_txcomp_batch): per id slice, how far the
// payload must reach, the leaf buffer it needs, and its items per tx.
// The payload crosses PCIe as two windows: the low one [0, low_end) -- the
// payloads below `split`, in practice those every transaction shares (the
// notary Party, TransactionType), written first -- once with the first slice,
// and the high one [high_min, pay_end[j]) growing slice by slice. Any split
// covers every item (an item lies below it or not); taking it at the shard's
// first transaction's last payload makes the high window start at this shard's
// own payloads, so a device of a multi-device context no longer copies the
// earlier shards' payloads (r05 copied [0, pay_end) on every device).
struct CompPlan {
  const cordahip_txcomp_batch* c = nullptr;
  std::vector<uint64_t> pay_end;  // high-window bytes slices 0..j reference (running max)
  std::vector<uint32_t> group;    // items per transaction when uniform in the slice (the encoder's hint), else 1
  uint64_t slice_cap = 16;        // leaf bytes of the largest piece's bound (the full chain's one leaf buffer)
  std::vector<std::vector<uint64_t>> cuts;  // per slice: the transactions that start a new piece of the full chain
  uint64_t max_items = 0;
  uint64_t split = 0;             // items at offsets below it are the low window's
  uint64_t low_end = 0;           // the low window [0, low_end)
  uint64_t high_min = UINT64_MAX; // the high window's first byte
  uint64_t copied = 0;            // high window enqueued up to here (from high_min)
  bool low_copied = false;
  bool templates_only = false;    // the steady-state encoder chain (misses redo the call)
  static constexpr uint64_t kDirectWriters = kKryoDirectWriters;  // the direct encoder's writers (rarely any work)
};

hipError_t tx_ids_prepare(cordahip_ctx* ctx, Device& d, TxSet& S, int set_idx, const cordahip_txid_batch* b,
                          const std::vector<uint64_t>& bound, CompPlan* cp) {
  const uint64_t t0 = bound.front(), t1 = bound.back(), ntx = t1 - t0;
  const uint64_t l0 = b->tx_leaf_off[t0], l1 = b->tx_leaf_off[t1], nleaves = l1 - l0;
  TxWork& w = S.tx;
  uint64_t leaf_buf = 0;
  if (cp) {
    const cordahip_txcomp_batch* c = cp->c;
    const size_t ns = bound.size() - 1;
    cp->pay_end.assign(ns, 0);
    cp->group.assign(ns, 1);
    cp->cuts.assign(ns, {});
    // the full chain's leaf buffer: a tenth of the device budget at most (the budget's
    // share for component slices; C4's 2^17-signature slices bound ~1.4 GB, far below
    // the default's 13.7 GB); a slice whose bound exceeds it is encoded and hashed in
    // pieces of whole transactions, one after another through the one buffer
    const uint64_t piece_cap = std::max<uint64_t>(d.mem_budget / 10, 1u << 20);
    std::vector<uint64_t> cap(ns, 0), low(ns, 0), hmin(ns, UINT64_MAX);
    auto fits = [&](const cordahip_kryo_item& it, uint64_t& off, uint64_t& nb) {
      off = (uint64_t)(uintptr_t)it.data;
      nb = comp_payload_bytes(it);
      return off <= c->payload_len && nb <= c->payload_len - off;
    };
    cp->split = 0;  // the shard's first transaction's last payload (its own, past the shared ones)
    for (uint64_t i = c->tx_item_off[t0]; i < c->tx_item_off[t0 + 1]; i++) {
      uint64_t off, nb;
      if (fits(c->items[i], off, nb) && nb) cp->split = std::max(cp->split, off);
    }
    pool_of(ctx, d).parallel_for(ns, 1, [&](uint64_t x, uint64_t y) {
      for (uint64_t j = x; j < y; j++) {
        const uint64_t ts0 = bound[j], ts1 = bound[j + 1];
        const uint64_t g = ts1 > ts0 ? c->tx_item_off[ts0 + 1] - c->tx_item_off[ts0] : 1;
        bool uniform = g > 0;
        uint64_t end = 0, bd = 0, lo_end = 0, hi_min = UINT64_MAX, piece_max = 0;
        for (uint64_t t = ts0; t < ts1; t++) {
          uniform = uniform && c->tx_item_off[t + 1] - c->tx_item_off[t] == g;
          const uint64_t bd_tx = bd;
          for (uint64_t i = c->tx_item_off[t]; i < c->tx_item_off[t + 1]; i++) {
            const cordahip_kryo_item& it = c->items[i];
            uint64_t off, nb;
            const bool ok = fits(it, off, nb);
            if (it.kind != CORDAHIP_KRYO_RAW && nb == 0) {
              bd += comp_leaf_bound(0);
              continue;
            }
            if (ok) {
              if (off < cp->split) {
                lo_end = std::max(lo_end, off + nb);
              } else {
                hi_min = std::min(hi_min, off);
                end = std::max(end, off + nb);
              }
            }
            bd += comp_leaf_bound(ok ? nb : 0);
          }
          if (bd > piece_cap && bd_tx > 0 && t > ts0) {  // t starts a new piece
            cp->cuts[j].push_back(t);
            piece_max = std::max(piece_max, bd_tx);
            bd -= bd_tx;
          }
        }
        cp->pay_end[j] = end;
        low[j] = lo_end;
        hmin[j] = hi_min;
        cp->group[j] = uniform && g <= 64 ? (uint32_t)g : 1;
        cap[j] = std::max(piece_max, bd);
      }
    });
    cp->low_end = 0;
    cp->high_min = UINT64_MAX;
    for (size_t j = 0; j < ns; j++) {
      cp->low_end = std::max(cp->low_end, low[j]);
      cp->high_min = std::min(cp->high_min, hmin[j]);
    }
    if (cp->high_min == UINT64_MAX) cp->high_min = 0;
    for (size_t j = 0; j < ns; j++) {
      if (j) cp->pay_end[j] = std::max(cp->pay_end[j], cp->pay_end[j - 1]);
      cp->slice_cap = std::max(cp->slice_cap, cap[j]);
      cp->max_items = std::max(cp->max_items, b->tx_leaf_off[bound[j + 1]] - b->tx_leaf_off[bound[j]]);
    }
    cp->copied = cp->high_min;
    cp->low_copied = false;
    // the templates-only chain hashes the leaves from their templates: no leaf buffers
    // (the full chain's leaf buffer is bounded at 4 KB + 4 B per payload byte per
    // component of its largest piece: ~1.4 GB for C4's 2^17-signature slices)
    cp->templates_only = cp->templates_only && d.kryo_templates_ok;
    if (w.comp_items.ensure(std::max<uint64_t>(nleaves, 1) * sizeof(cordahip_kryo_item)) ||
        w.payload.ensure(std::max<uint64_t>(std::max(ns ? cp->pay_end.back() : 0, cp->low_end), 16)) ||
        w.comp_status.ensure(std::max<uint64_t>(nleaves, 1)))
      return hipErrorOutOfMemory;
    // the encoder's scratch (d.kryo_*, kryo_mu held by the caller) for the largest slice
    const uint64_t n = cp->max_items;
    size_t temp_bytes = 0;
    if (hipError_t e = kryo_scan_bytes(temp_bytes, n + 1, d.stream)) return e;
    if (hipError_t e = kryo_scratch_ensure(d, n, std::max<size_t>(temp_bytes, 16))) return e;
    if (hipError_t e = usage_buffer(S.kryo_usage, S.kryo_usage_dev)) return e;
    if (hipError_t e = kryo_state_ready(d, d.stream)) return e;
    if (hipError_t e = kryo_reset_misses(d.kryo_fixed.as<uint8_t>(), (uint32_t)set_idx, d.stream)) return e;
    cp->templates_only = cp->templates_only && d.kryo_templates_ok;  // kryo_state_ready may have cleared the table
    // sized after that: a cleared table runs the full chain, which writes leaves
    leaf_buf = cp->templates_only ? 0 : cp->slice_cap;
    if (tracing())
      fprintf(stderr, "[cordahip] dev %d set %d component call: %s chain (templates %u, slots %u in use)\n", d.id,
              set_idx, cp->templates_only ? "templates-only" : "full encoder", S.kryo_usage.as<uint32_t>()[0],
              S.kryo_usage.as<uint32_t>()[1]);
  } else {
    leaf_buf = b->leaf_off[l1] - b->leaf_off[l0];
  }
  if (w.leaf_bytes.ensure(std::max<uint64_t>(leaf_buf, 16)) || w.leaf_off.ensure((nleaves + 1) * 8) ||
      w.tx_leaf_off.ensure((ntx + 1) * 8) || w.hashes.ensure(std::max<uint64_t>(nleaves, 1) * 32) ||
      w.txid.ensure(std::max<uint64_t>(ntx, 1) * 32) || w.tx_status.ensure(std::max<uint64_t>(ntx, 1)))
    return hipErrorOutOfMemory;
  return hipSuccess;
}

hipError_t tx_ids_enqueue(Device& d, TxSet& S, int set_idx, const cordahip_txid_batch* b,
                          const std::vector<uint64_t>& bound, size_t j0, size_t j1, std::vector<hipEvent_t>& ev,
                          std::vector<hipEvent_t>& cev, std::vector<hipEvent_t>& kev, uint8_t* map_txid,
                          uint8_t* map_status, CompPlan* cp) {
  const uint64_t t0 = bound.front();
  const uint64_t l0 = b->tx_leaf_off[t0], b0 = cp ? 0 : b->leaf_off[l0];
  TxWork& w = S.tx;
  hipStream_t s = d.stream, sc = d.s_idcopy ? d.s_idcopy : d.stream;
  const hipMemcpyKind h2d = hipMemcpyHostToDevice, d2h = hipMemcpyDeviceToHost;
  const uint8_t* bytes_base = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(w.leaf_bytes.p) - b0);
  uint32_t* hash_base = reinterpret_cast<uint32_t*>(reinterpret_cast<uintptr_t>(w.hashes.p) - l0 * 32);
  hipError_t e = hipSuccess;
  for (size_t j = j0; j < j1 && e == hipSuccess; j++) {
    const uint64_t ts0 = bound[j], ts1 = bound[j + 1];
    const uint64_t ls0 = b->tx_leaf_off[ts0], ls1 = b->tx_leaf_off[ts1];
    if (!cp) {
      const uint64_t bs0 = b->leaf_off[ls0], bs1 = b->leaf_off[ls1];
      if (bs1 > bs0)
        e = blocked("leaf-bytes H2D", [&] {
          return hipMemcpyAsync(w.leaf_bytes.as<uint8_t>() + (bs0 - b0), b->leaf_bytes + bs0, bs1 - bs0, h2d, sc);
        });
      e = e ? e : hipMemcpyAsync(w.leaf_off.as<uint64_t>() + (ls0 - l0), b->leaf_off + ls0, (ls1 - ls0 + 1) * 8, h2d, sc);
    } else {
      // the slice's components, and the payload prefix they reach
      const cordahip_txcomp_batch* c = cp->c;
      if (ls1 > ls0)
        e = hipMemcpyAsync(w.comp_items.as<cordahip_kryo_item>() + (ls0 - l0), c->items + ls0,
                           (ls1 - ls0) * sizeof(cordahip_kryo_item), h2d, sc);
      if (e == hipSuccess && !cp->low_copied) {  // the low window, once (the shared payloads)
        cp->low_copied = true;
        if (cp->low_end)
          e = hipMemcpyAsync(w.payload.as<uint8_t>(), c->payload, cp->low_end, h2d, sc);
      }
      if (e == hipSuccess && cp->pay_end[j] > cp->copied) {  // the high window grows with the slices
        e = blocked("payload H2D", [&] {
          return hipMemcpyAsync(w.payload.as<uint8_t>() + cp->copied, c->payload + cp->copied,
                                cp->pay_end[j] - cp->copied, h2d, sc);
        });
        cp->copied = cp->pay_end[j];
      }
    }
    e = e ? e : hipMemcpyAsync(w.tx_leaf_off.as<uint64_t>() + (ts0 - t0), b->tx_leaf_off + ts0, (ts1 - ts0 + 1) * 8, h2d, sc);
    e = e ? e : hipEventRecord(cev[j], sc);
    e = e ? e : hipStreamWaitEvent(s, cev[j], 0);
    if (cp && cp->templates_only) {
      // steady state: shapes, then every leaf's SHA-256 straight from its template
      // (no leaf bytes in HBM)
      uint32_t* slots = d.kryo_items.as<uint32_t>();
      const uint64_t n = ls1 - ls0;
      const cordahip_kryo_item* it = w.comp_items.as<cordahip_kryo_item>() + (ls0 - l0);
      uint8_t* cst = w.comp_status.as<uint8_t>() + (ls0 - l0);
      // shapes and hashes in one launch per slice (the shape pass inside kryo_hash's
      // template-grouped blocks): c4h --components at two calls in flight 88.7-90.1 ->
      // 91.3-92.1 M sig/s, alternating on one box (profiles/r06_kryo_fused_ab/);
      // CORDAHIP_KRYO_FUSED=0: the two launches
      static const bool fused = !(getenv("CORDAHIP_KRYO_FUSED") && getenv("CORDAHIP_KRYO_FUSED")[0] == '0');
      if (fused) {
        e = e ? e : launch_kryo_shape_hash(it, w.payload.as<uint8_t>(), cp->c->payload_len, n, cp->group[j],
                                           d.kryo_fixed.as<uint8_t>(), cst, w.hashes.as<uint32_t>() + (ls0 - l0) * 8,
                                           s, (uint32_t)set_idx);
      } else {
        e = e ? e : launch_kryo_shape(it, w.payload.as<uint8_t>(), cp->c->payload_len, n, cp->group[j],
                                      d.kryo_fixed.as<uint8_t>(), slots, slots + n, d.kryo_sizes.as<uint64_t>(), cst, s,
                                      true, (uint32_t)set_idx);
        e = e ? e : launch_kryo_hash(it, w.payload.as<uint8_t>(), cp->c->payload_len, n, cp->group[j],
                                     d.kryo_fixed.as<uint8_t>(), slots, d.kryo_sizes.as<uint64_t>(), cst,
                                     w.hashes.as<uint32_t>() + (ls0 - l0) * 8, s);
      }
    } else if (cp) {
      // the slice's leaves on the GPU (the template encoder) into the leaf buffer,
      // offsets relative to it, then their SHA-256; piece by piece (whole
      // transactions) when the slice's bound exceeds the buffer. Every piece runs
      // on s, so the next piece's writes follow the previous piece's hashing.
      uint8_t* sb = w.leaf_bytes.as<uint8_t>();
      uint32_t* slots = d.kryo_items.as<uint32_t>();
      uint64_t pa = ts0;
      for (size_t k = 0; k <= cp->cuts[j].size() && e == hipSuccess; k++) {
        const uint64_t pb = k < cp->cuts[j].size() ? cp->cuts[j][k] : ts1;
        const uint64_t is0 = b->tx_leaf_off[pa], n = b->tx_leaf_off[pb] - is0;
        pa = pb;
        if (!n) continue;
        e = launch_kryo_encode(w.comp_items.as<cordahip_kryo_item>() + (is0 - l0), w.payload.as<uint8_t>(),
                               cp->c->payload_len, n, cp->group[j], d.kryo_fixed.as<uint8_t>(), slots, slots + n,
                               d.kryo_sizes.as<uint64_t>(), w.leaf_off.as<uint64_t>() + (is0 - l0), sb, cp->slice_cap,
                               w.comp_status.as<uint8_t>() + (is0 - l0), d.kryo_ws.as<uint8_t>(),
                               CompPlan::kDirectWriters, d.kryo_temp.p, d.kryo_temp.cap, s, cp->templates_only,
                               (uint32_t)set_idx);
        e = e ? e : launch_sha256_leaves(sb, w.leaf_off.as<uint64_t>() + (is0 - l0), n,
                                         w.hashes.as<uint32_t>() + (is0 - l0) * 8, s);
      }
    } else {
      e = e ? e : blocked("sha256_leaves launch", [&] {
        return launch_sha256_leaves(bytes_base, w.leaf_off.as<uint64_t>() + (ls0 - l0), ls1 - ls0,
                                    w.hashes.as<uint32_t>() + (ls0 - l0) * 8, s);
      });
    }
    // the ids, and in the same launch: a component the encoder rejected (no id for its
    // transaction, CORDAHIP_TX_BAD_COMPONENT) and the stores into pinned caller arrays
    // through their device mapping (three launches per slice before r05)
    const uint8_t* st_base =
        cp ? reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(w.comp_status.p) - l0) : nullptr;
    const bool mapped = ts1 > ts0 && map_txid && map_status;
    e = e ? e : launch_merkle_root(hash_base, w.tx_leaf_off.as<uint64_t>() + (ts0 - t0), ts1 - ts0,
                                   w.txid.as<uint8_t>() + (ts0 - t0) * 32, w.tx_status.as<uint8_t>() + (ts0 - t0), s,
                                   st_base, mapped ? map_txid + ts0 * 32 : nullptr, mapped ? map_status + ts0 : nullptr);
    e = e ? e : hipEventRecord(kev[j], s);  // the slice's ids are in HBM: its signatures may gather them
    if (mapped) {
      // stored by merkle_root
    } else if (ts1 > ts0) {
      e = e ? e : blocked("ids D2H", [&] {
        return hipMemcpyAsync(b->txid + ts0 * 32, w.txid.as<uint8_t>() + (ts0 - t0) * 32, (ts1 - ts0) * 32, d2h, s);
      });
      e = e ? e : blocked("id status D2H", [&] {
        return hipMemcpyAsync(b->tx_status + ts0, w.tx_status.as<uint8_t>() + (ts0 - t0), ts1 - ts0, d2h, s);
      });
    }
    e = e ? e : hipEventRecord(ev[j], s);
  }
  if (e == hipSuccess && j1 + 1 == bound.size()) {
    // the last slice: the encoder's usage report, then the fences of the set's
    // buffers (S.tx_ev: the call's drain waits on it) and of the encoder's
    // scratch (d.kryo_*)
    if (cp) e = kryo_usage_report(d, &S, s);
    e = e ? e : S.tx_ev.record(s);
    if (cp) e = e ? e : d.kryo_ev.record(s);
  }
  return e;
}

// The per-transaction verdict of txs [t0, t1) from their id statuses and
// signature statuses (SignedTransaction.verifySignaturesExcept -> the first
// signature that fails, SignedTransaction.kt:95-100): first_bad_sig, and the
// tx status becomes that signature's status.
//
// cover != nullptr (the _covered calls): the same worker then runs the
// required-signer coverage of its transactions (cover_core.hpp tx_eval: the
// second half of verifySignatures, getMissingSignatures :102-108) -- their
// statuses and signature keys are in its cache, and the cover arrays never
// cross PCIe to bring back one byte. A transaction is reduced exactly once
// (the chunks' ranges and the final sweep are disjoint), which coverage needs:
// it reads the status it may then overwrite.
void reduce_txs(HostPool& pool, const cordahip_signed_tx_batch* b, uint64_t t0, uint64_t t1,
                const cordahip_cover* cover = nullptr, std::atomic<bool>* cover_oom = nullptr) {
  if (t0 >= t1) return;
  pool.parallel_for(t1 - t0, 4096, [&](uint64_t x, uint64_t y) {
    for (uint64_t t = t0 + x; t < t0 + y; t++) {
      const uint64_t lo = b->tx_sig_off[t], hi = b->tx_sig_off[t + 1];
      b->first_bad_sig[t] = -1;
      if (lo == hi) {  // require(sigs.isNotEmpty()) in the constructor (SignedTransaction.kt:37-39) precedes tx.id
        b->tx.tx_status[t] = CORDAHIP_TX_NO_SIGNATURES;
        continue;
      }
      if (b->tx.tx_status[t] != CORDAHIP_STATUS_OK) {  // tx.id threw before any signature was checked
        for (uint64_t s = lo; s < hi; s++) b->sig_status[s] = b->tx.tx_status[t];
        continue;
      }
      for (uint64_t s = lo; s < hi; s++)
        if (b->sig_status[s] != CORDAHIP_STATUS_OK) {
          b->first_bad_sig[t] = (int64_t)(s - lo);
          b->tx.tx_status[t] = b->sig_status[s];
          break;
        }
    }
    if (!cover) return;
    const cover::SigKeysCsr sig{b->scheme, b->key, b->key_off};
    cover::LocalStack stack;  // inline for trees of up to 64 tokens, the heap beyond
    for (uint64_t t = t0 + x; t < t0 + y; t++) cover::tx_eval(*cover, t, b->tx.tx_status, b->tx_sig_off, sig, stack);
    if (stack.failed && cover_oom) cover_oom->store(true);
  });
}

// SignedTransaction.checkSignaturesAreValid over the batch: tx ids (K3/K4),
// every signature over its tx's id (the generic signature pipeline), then the
// per-tx first failing signature. Each device takes a contiguous shard of the
// transactions AND their signatures (a transaction's leaves and signatures stay
// on one GPU). Its ids are computed in slices (tx_ids_enqueue: slice
// j + 1's leaf bytes cross PCIe on their own stream while slice j hashes), each
// slice marking an event when its ids are in HBM. The signature pipeline runs
// over the shard's signatures in chunks of one or more whole slices: it packs
// and copies keys and signatures without waiting for any id -- they do not
// depend on the ids -- plus each row's id index, and the GPU gathers the message
// rows from the ids in HBM after the slice's event (gather_rows32). Slices are
// released just ahead of the chunk that needs them and `lookahead` more after
// its copies (DeviceIds::advance), so the DMA engine, which serves H2D copies in
// submission order, interleaves leaf bytes and signature chunks. The ids go to
// the caller (txid) on the side; no signature waits for an id to reach the
// host. (r03 waited for each slice's ids on the host and copied them back as
// messages: the GPU sat idle ~5 ms per C4 step until the first signatures were
// packed.)
// Consecutive calls on one device overlap (r06): a call holds one of the
// device's two buffer sets (SetLease: ids, leaf / component buffers, the
// signature stages) from start to finish, but the device's enqueue token
// (tx_order_mu) -- and, for component batches, the encoder's scratch lock
// (kryo_mu) -- only until its last signature chunk and id slice are enqueued.
// The next call then packs and enqueues its first slices and chunks while this
// one drains (its last chunks' ladders, the statuses, the per-tx reduce), so
// the GPU no longer idles through each call's fill (the first slice's leaf
// bytes and pack) and drain. Work reaches the shared streams in call order; a
// call's drain waits on its own events, never on the streams.
constexpr int kRedoFull = -1000;  // a templates-only component call missed: run it again with the full encoder

int signed_tx_device_once(cordahip_ctx* ctx, Device& d, const cordahip_signed_tx_batch* b, uint64_t* tx_of,
                          uint64_t lo, uint64_t hi, uint64_t slices, const cordahip_txcomp_batch* comps,
                          bool templates_only, const cordahip_cover* cover) {
  SetLease lease(d);  // S.tx (the ids) and S.pb stay ours until every gather has run
  TxSet& S = lease.get();
  const int set_idx = lease.index();
  const NodeBind nb(d);  // this thread packs and first-touches on the GPU's NUMA node
  const Activity act(d);
  std::unique_lock<std::mutex> tok(d.tx_order_mu);
  // component batches also enqueue on the GPU encoder's shared scratch (d.kryo_*)
  std::unique_lock<std::mutex> gk(d.kryo_mu, std::defer_lock);
  CompPlan plan, *cp = nullptr;
  uint64_t gen = 0;
  if (comps) {
    gk.lock();
    plan.c = comps;
    plan.templates_only = templates_only;
    cp = &plan;
  }
  int r = tx_acquire_host(d, S);
  if (r == CORDAHIP_SUCCESS && ensure_streams(d) != hipSuccess) r = CORDAHIP_ERR_HIP;
  if (r == CORDAHIP_SUCCESS && cp && d.kryo_ev.wait(d.stream) != hipSuccess)
    r = CORDAHIP_ERR_HIP;  // an earlier cordahip_kryo_encode_device still using the scratch
  if (r != CORDAHIP_SUCCESS) return r;
  DeviceIds di;
  std::atomic<bool> cover_oom{false};  // a coverage worker could not get its stack (reduce_txs)
  const uint64_t s0 = b->tx_sig_off[lo], s1 = b->tx_sig_off[hi];
  // signature chunks of whole full-occupancy rounds of the Ed25519 ladder
  // (2^17 lanes: 2 waves x 1,024 SIMDs x 64), each waiting on device for the
  // slice that holds its last transaction. r04 ran half rounds (2^16: the GPU
  // starts after the leaf bytes of fewer transactions, and two Ed25519 streams
  // keep two chunks in flight so one chunk's tail overlaps the next). Since the
  // id kernels run at raised wave priority (tx.hip g_id_prio) a slice's ids no
  // longer trail the ladders, and whole rounds win: interleaved on one corpus,
  // c4h 84.1 against 81.6 M sig/s, c4h --components 75.0 against 72.3; 2^18:
  // 70.3 (profiles/r05_c4h_chunk_ab/).
  uint64_t chunk = 1u << 17;
  if (const char* v = getenv("CORDAHIP_TX_SIG_CHUNK")) chunk = std::max<uint64_t>(1, strtoull(v, nullptr, 10));
  // chunks double from `chunk` up to CORDAHIP_TX_SIG_CHUNK_MAX (default: chunk,
  // constant chunks; 2^16 doubling to 2^17 ran 83.9 against 84.1 M/s, r05)
  uint64_t chunk_max = chunk;
  if (const char* v = getenv("CORDAHIP_TX_SIG_CHUNK_MAX")) chunk_max = std::max<uint64_t>(chunk, strtoull(v, nullptr, 10));
  for (uint64_t x = s0, c = chunk; x < s1; x += c, c = std::min(chunk_max, 2 * c)) di.chunk_bound.push_back(x);
  di.chunk_bound.push_back(s1);
  if (slices == 0 && s1 > s0) {
    // default: the id slices follow the chunks -- slice k ends with chunk k's
    // last transaction, so chunk k waits for exactly its own ids, and the first
    // slice's leaf bytes (what the GPU waits for before its first ladder) are
    // one round's worth, not a sixteenth of the shard (r04_n trace: 1.1 ms of
    // PCIe before the first kernel)
    di.tx_bound.push_back(lo);
    for (size_t c = 1; c + 1 < di.chunk_bound.size(); c++) {
      // one past the transaction holding the chunk's last signature (tx_of is
      // not filled yet: it is built while slice 0 crosses PCIe)
      const uint64_t t = (uint64_t)(std::upper_bound(b->tx_sig_off + lo, b->tx_sig_off + hi + 1,
                                                     di.chunk_bound[c] - 1) - b->tx_sig_off);
      if (t > di.tx_bound.back() && t < hi) di.tx_bound.push_back(t);
    }
    di.tx_bound.push_back(hi);
    slices = di.tx_bound.size() - 1;
  } else {  // CORDAHIP_TX_SLICES, or no signatures: uniform slices
    slices = std::max<uint64_t>(1, std::min<uint64_t>(slices ? slices : 1, hi - lo));
    for (uint64_t q = 0; q <= slices; q++) di.tx_bound.push_back(lo + (hi - lo) * q / slices);
  }
  std::vector<hipEvent_t> ev(slices, nullptr), cev(slices, nullptr);
  di.ready.assign(slices, nullptr);
  struct Events {  // destroyed on every exit
    std::vector<hipEvent_t>* v[3];
    ~Events() {
      for (auto* x : v)
        for (hipEvent_t e : *x)
          if (e) (void)hipEventDestroy(e);
    }
  } events{{&ev, &cev, &di.ready}};
  for (auto* v : {&ev, &cev, &di.ready})
    for (auto& e : *v)
      if (r == CORDAHIP_SUCCESS && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) r = CORDAHIP_ERR_HIP;
  // slices go out a few ahead of the signature chunk that needs them (the
  // chunk's own H2D follows them through the DMA engine in submission order):
  // with every slice enqueued first, r04's first signature copies waited ~20 ms
  // behind all of C4's 1.05 GB of leaf bytes
  size_t issued = 0;
  uint8_t* map_txid = static_cast<uint8_t*>(host_mapped(b->tx.txid));
  uint8_t* map_status = static_cast<uint8_t*>(host_mapped(b->tx.tx_status));
  uint64_t lookahead = 1;  // r04_o: 1 slice ahead 73.6 M/s, 2 ahead 73.1
  if (const char* v = getenv("CORDAHIP_TX_SLICE_AHEAD")) lookahead = strtoull(v, nullptr, 10);
  auto issue_through = [&](size_t j) -> hipError_t {  // enqueue slices [issued, j]
    const size_t j1 = std::min<size_t>(slices, j + 1);
    hipError_t e = hipSuccess;
    if (j1 > issued)
      e = tx_ids_enqueue(d, S, set_idx, &b->tx, di.tx_bound, issued, j1, ev, cev, di.ready, map_txid, map_status, cp);
    issued = std::max(issued, j1);
    return e;
  };
  // the end of this call's enqueues: the slices no signature asked for
  // (transactions without signatures at the end), then the token and the
  // encoder's scratch go to the next call (idempotent: called by the pipeline
  // once its last chunk is enqueued, and after it)
  bool handed_on = false;
  auto hand_on = [&]() -> hipError_t {
    if (handed_on) return hipSuccess;
    handed_on = true;
    const hipError_t e = issue_through(slices);
    if (gk.owns_lock()) gk.unlock();
    if (tok.owns_lock()) tok.unlock();
    return e;
  };
  if (r == CORDAHIP_SUCCESS && tx_ids_prepare(ctx, d, S, set_idx, &b->tx, di.tx_bound, cp) != hipSuccess)
    r = CORDAHIP_ERR_OUT_OF_MEMORY;
  if (cp) gen = d.kryo_gen;  // after a clear in prepare: this call builds the new table's shapes
  if (r == CORDAHIP_SUCCESS && issue_through(0) != hipSuccess) r = CORDAHIP_ERR_HIP;
  // each signature signs its transaction's id (SignedTransaction.kt:98): the
  // pipeline finds it through tx_of, filled chunk by chunk just ahead of its use
  // (fill_to, from di.advance) -- built whole before the first chunk it held the
  // first pack ~0.5 ms (r05 host trace: C4's 2.5 M signatures)
  uint64_t filled = s0;  // tx_of holds signatures [s0, filled)
  auto fill_to = [&](uint64_t s_end) {
    s_end = std::min(s_end, s1);
    if (s_end <= filled) return;
    const uint64_t* so = b->tx_sig_off;
    const uint64_t ta = (uint64_t)(std::upper_bound(so + lo, so + hi + 1, filled) - so) - 1;
    const uint64_t tb = (uint64_t)(std::upper_bound(so + lo, so + hi + 1, s_end - 1) - so);
    const uint64_t f0 = filled;
    pool_of(ctx, d).parallel_for(tb - ta, 4096, [&](uint64_t x, uint64_t y) {
      for (uint64_t t = ta + x; t < ta + y; t++)
        for (uint64_t q = std::max(so[t], f0); q < std::min(so[t + 1], s_end); q++) tx_of[q] = t;
    });
    filled = s_end;
  };
  std::vector<std::pair<uint64_t, uint64_t>> reduced;  // tx ranges the chunks reduced
  if (r == CORDAHIP_SUCCESS && s1 > s0) {
    di.txid = S.tx.txid.as<uint8_t>();
    di.t0 = lo;
    // CORDAHIP_TX_SPLIT_PREP (A/B): 0 fused prep everywhere, 1 split for component batches
    // too; default split for leaf batches only (r05, profiles/r05_prep_split_ab/)
    static const int split_env = getenv("CORDAHIP_TX_SPLIT_PREP") ? atoi(getenv("CORDAHIP_TX_SPLIT_PREP")) : -1;
    di.split_prep = split_env < 0 ? cp == nullptr : split_env > 0;
    // before a chunk's copies: the slices it needs; after them: `lookahead` more,
    // so PCIe carries leaf bytes while the GPU verifies the chunk
    di.advance = [&](uint64_t sig_end, bool after) {
      // after: the slices of the next `lookahead` chunks' signatures
      const uint64_t e = after ? std::min(s1, sig_end + lookahead * chunk_max) : sig_end;
      fill_to(e);
      const uint64_t tx = tx_of[e - 1];
      const size_t j = (size_t)(std::upper_bound(di.tx_bound.begin(), di.tx_bound.end(), tx) - di.tx_bound.begin()) - 1;
      return issue_through(j);
    };
    di.enqueued = hand_on;
    // each finished chunk reduces the transactions whose signatures it holds
    // entirely (once their ids are on the host), overlapped with later chunks'
    // GPU work: the whole-batch pass after the drain was ~0.55 ms of a 32 ms
    // C4 call with the GPU idle; edge transactions are reduced after the drain
    di.done = [&](uint64_t a, uint64_t e) -> hipError_t {
      uint64_t t0 = tx_of[a], t1 = tx_of[e - 1];
      if (b->tx_sig_off[t0] != a) t0++;       // starts in an earlier chunk
      if (b->tx_sig_off[t1 + 1] == e) t1++;   // ends here: included
      if (t0 >= t1) return hipSuccess;
      const size_t j0 = (size_t)(std::upper_bound(di.tx_bound.begin(), di.tx_bound.end(), t0) - di.tx_bound.begin()) - 1;
      const size_t j1 = (size_t)(std::upper_bound(di.tx_bound.begin(), di.tx_bound.end(), t1 - 1) - di.tx_bound.begin());
      for (size_t j = j0; j < j1; j++) {  // their slices' ids and statuses are back (issued: the chunk needed them)
        if (j >= issued) return hipErrorInvalidValue;
        if (hipError_t x = blocked("ids on the host", [&] { return hipEventSynchronize(ev[j]); })) return x;
      }
      const double tr = tracing() ? now_ms() : 0;
      reduce_txs(pool_of(ctx, d), b, t0, t1, cover, &cover_oom);
      if (tracing() && now_ms() - tr > 1.0) fprintf(stderr, "[cordahip] reduce of %llu txs %.2f ms\n",
                                                    (unsigned long long)(t1 - t0), now_ms() - tr);
      reduced.push_back({t0, t1});
      return hipSuccess;
    };
    MsgView mv{b->tx.txid, nullptr, tx_of};
    mv.dev = &di;
    // checkSignaturesAreValid -> sig.verify -> Crypto.doVerify: doVerify semantics. The
    // struct carries no flags: cordahip_set_rsa_on_device stands for CORDAHIP_FLAG_RSA_ON_DEVICE
    const uint32_t sig_flags = ctx->rsa_on_device.load(std::memory_order_relaxed) ? CORDAHIP_FLAG_RSA_ON_DEVICE : 0u;
    cordahip_sig_batch sb{b->tx_sig_off[b->tx.ntx], b->scheme, b->key, b->key_off, b->sig, b->sig_off, b->tx.txid,
                          nullptr, b->sig_status, nullptr, sig_flags, b->key_bytes, b->sig_bytes, 0};
    try {
      r = sig_verify_range(ctx, d, S, &sb, mv, s0, s1);
    } catch (const std::bad_alloc&) {
      r = CORDAHIP_ERR_OUT_OF_MEMORY;
    } catch (...) {
      r = CORDAHIP_ERR_HIP;
    }
  }
  const double tr0 = tracing() ? now_ms() : 0;
  // slices no signature asked for; the token goes on (if the pipeline did not hand
  // it on; after an error nothing more is enqueued)
  if (r == CORDAHIP_SUCCESS) {
    if (hand_on() != hipSuccess) r = CORDAHIP_ERR_HIP;
  } else {
    handed_on = true;
    if (gk.owns_lock()) gk.unlock();
    if (tok.owns_lock()) tok.unlock();
  }
  // every slice writes the caller's txid / tx_status: drain before returning,
  // errors included. S.tx_ev follows the last slice (and the encoder's usage
  // report) on the id stream, after every earlier slice; the id copies on
  // s_idcopy precede their slices' kernels. After an error the streams
  // themselves are drained.
  hipError_t e1 = hipSuccess;
  if (r == CORDAHIP_SUCCESS) e1 = S.tx_ev.sync();
  if (r != CORDAHIP_SUCCESS || e1 != hipSuccess) {
    (void)hipStreamSynchronize(d.s_idcopy ? d.s_idcopy : d.stream);
    (void)hipStreamSynchronize(d.stream);
  }
  const double tr1 = tracing() ? now_ms() : 0;
  if (r == CORDAHIP_SUCCESS && e1 != hipSuccess) r = CORDAHIP_ERR_HIP;
  if (r != CORDAHIP_SUCCESS) return r;
  if (cp) {
    // the encoder's misses in this call (this set's counter, reported after its last
    // slice, drained above): a templates-only call with any is void; a full call
    // without any lets the next call on this device take the templates-only chain
    const uint32_t misses = static_cast<const volatile uint32_t*>(S.kryo_usage.as<uint32_t>())[2 + set_idx];
    if (tracing()) fprintf(stderr, "[cordahip] dev %d set %d component call: %u encoder misses\n", d.id, set_idx, misses);
    std::lock_guard<std::mutex> g(d.kryo_mu);
    if (cp->templates_only && misses) {
      d.kryo_templates_ok = false;
      return kRedoFull;
    }
    if (d.kryo_gen == gen) d.kryo_templates_ok = misses == 0;
  }
  // the transactions no chunk reduced: chunk-edge ones, those without signatures
  std::sort(reduced.begin(), reduced.end());
  uint64_t t = lo;
  for (const auto& rg : reduced) {
    reduce_txs(pool_of(ctx, d), b, t, rg.first, cover, &cover_oom);
    t = std::max(t, rg.second);
  }
  reduce_txs(pool_of(ctx, d), b, t, hi, cover, &cover_oom);
  if (cover_oom.load()) r = CORDAHIP_ERR_OUT_OF_MEMORY;
  if (tracing())
    fprintf(stderr, "[cordahip] dev %d signed tx tail: id streams drained %.2f ms, edge reduce %.2f ms\n", d.id,
            tr1 - tr0, now_ms() - tr1);
  return r;
}

// A component batch runs the encoder's templates-only chain when the device's
// last component batch needed no new template and no direct encoder
// (Device::kryo_templates_ok): per id slice, the shape pass and the leaf hashes
// straight from the templates (kryo_hash: no leaf bytes), without the build /
// size / direct-write kernels whose empty launches sat on each slice's critical
// path. An item that would need them is a miss; the call
// then runs again with the full chain (its results overwrite every output).
// CORDAHIP_KRYO_TEMPLATES_ONLY=0 always runs the full chain.
int signed_tx_device(cordahip_ctx* ctx, Device& d, const cordahip_signed_tx_batch* b, uint64_t* tx_of, uint64_t lo,
                     uint64_t hi, uint64_t slices, const cordahip_txcomp_batch* comps, const cordahip_cover* cover) {
  static const bool spec = [] {
    const char* v = getenv("CORDAHIP_KRYO_TEMPLATES_ONLY");
    return !(v && v[0] == '0');
  }();
  const int r = signed_tx_device_once(ctx, d, b, tx_of, lo, hi, slices, comps, comps && spec, cover);
  if (r == kRedoFull && tracing())
    fprintf(stderr, "[cordahip] dev %d component call: templates-only chain missed, redone with the full encoder\n",
            d.id);
  return r == kRedoFull ? signed_tx_device_once(ctx, d, b, tx_of, lo, hi, slices, comps, false, cover) : r;
}

// cover != nullptr: the _covered forms (required-signer coverage after each reduce)
int signed_tx_impl(cordahip_ctx* ctx, const cordahip_signed_tx_batch* b, const cordahip_txcomp_batch* comps = nullptr,
                   const cordahip_cover* cover = nullptr) {
  const uint64_t ntx = b->tx.ntx;
  if (ntx == 0) return CORDAHIP_SUCCESS;
  if (!b->tx_sig_off || !b->first_bad_sig || !b->sig_status) return CORDAHIP_ERR_INVALID_ARG;
  if (comps) {  // components instead of leaves (b->tx.tx_leaf_off = comps->tx_item_off)
    if (!comps->tx_item_off || !comps->txid || !comps->tx_status || (comps->tx_item_off[ntx] && !comps->items) ||
        (comps->payload_len && !comps->payload))
      return CORDAHIP_ERR_INVALID_ARG;
  } else if (!b->tx.leaf_off || !b->tx.tx_leaf_off || !b->tx.txid || !b->tx.tx_status || !b->tx.leaf_bytes) {
    return CORDAHIP_ERR_INVALID_ARG;
  }
  // the CSR levels (csr_check.hpp), whole, before any enqueue: the leaves or the
  // items, then the signatures
  const PoolPar par{*ctx->host};
  if (comps ? !check_txcomp_batch(par, comps) : !check_txid_batch(par, &b->tx)) return CORDAHIP_ERR_INVALID_ARG;
  if (!check_sig_level(par, ntx, b->tx_sig_off, b->nsig, b->key_off, b->key_bytes, b->sig_off, b->sig_bytes))
    return CORDAHIP_ERR_INVALID_ARG;
  if (cover && !check_cover(par, cover, ntx)) return CORDAHIP_ERR_INVALID_ARG;
  const uint64_t nsig = b->tx_sig_off[ntx];
  if (nsig && (!b->scheme || !b->key || !b->key_off || !b->sig || !b->sig_off)) return CORDAHIP_ERR_INVALID_ARG;
  const double t0 = tracing() ? now_ms() : 0;
  // signature -> transaction (tx_of), each device filling its shard's part
  // (signed_tx_device); the buffer comes from the context's cache and goes
  // back to it on every exit
  struct TxOf {
    cordahip_ctx* ctx;
    std::unique_ptr<uint64_t[]> p;
    uint64_t cap = 0;
    TxOf(cordahip_ctx* c, uint64_t n) : ctx(c) {
      std::lock_guard<std::mutex> g(ctx->txof_mu);
      auto& f = ctx->txof_free;
      for (size_t i = 0; i < f.size(); i++)
        if (f[i].second >= n) {
          p = std::move(f[i].first);
          cap = f[i].second;
          f.erase(f.begin() + (long)i);
          return;
        }
    }
    ~TxOf() {
      if (!p) return;
      std::lock_guard<std::mutex> g(ctx->txof_mu);
      auto& f = ctx->txof_free;
      if (f.size() < cordahip_ctx::kTxOfCache) f.emplace_back(std::move(p), cap);
    }
  } buf(ctx, nsig);
  if (!buf.p && nsig) {
    buf.p.reset(new uint64_t[nsig]);
    buf.cap = nsig;
  }
  uint64_t* tx_of = buf.p.get();
  const double t_of = tracing() ? now_ms() : 0;
  // per device: its contiguous tx shard in slices (CORDAHIP_TX_SLICES; default:
  // one slice per signature chunk) and, chunk by
  // chunk and after the drain, the per-transaction reduce (reduce_txs)
  uint64_t slices = 0;
  if (const char* v = getenv("CORDAHIP_TX_SLICES")) slices = std::max<uint64_t>(1, strtoull(v, nullptr, 10));
  const int rc = for_shards(ctx->devs, ntx, 1, [&](Device& d, uint64_t lo, uint64_t hi) {
    return signed_tx_device(ctx, d, b, tx_of, lo, hi, slices, comps, cover);
  });
  const double t_ids = tracing() ? now_ms() : 0;
  if (rc != CORDAHIP_SUCCESS) return rc;
  if (tracing())
    fprintf(stderr, "[cordahip] signed tx batch: %llu txs, %llu sigs, %llu id slices per device: tx_of %.2f ms, "
            "ids, signatures and reduce done at %.2f ms\n", (unsigned long long)ntx, (unsigned long long)nsig,
            (unsigned long long)slices, t_of - t0, t_ids - t0);  // slices 0: the per-device default
  return CORDAHIP_SUCCESS;
}

// cordahip_signed_txcomp_batch as the leaf-batch descriptor the pipeline reads
// (no leaf bytes: the slices encode them on the device), plus the components
int signed_txcomp_impl(cordahip_ctx* ctx, const cordahip_signed_txcomp_batch* cb, const cordahip_cover* cover = nullptr) {
  cordahip_signed_tx_batch b{};
  b.tx.ntx = cb->tx.ntx;
  b.tx.tx_leaf_off = cb->tx.tx_item_off;  // one leaf per component
  b.tx.txid = cb->tx.txid;
  b.tx.tx_status = cb->tx.tx_status;
  b.tx_sig_off = cb->tx_sig_off;
  b.scheme = cb->scheme;
  b.key = cb->key;
  b.key_off = cb->key_off;
  b.sig = cb->sig;
  b.sig_off = cb->sig_off;
  b.sig_status = cb->sig_status;
  b.first_bad_sig = cb->first_bad_sig;
  b.nsig = cb->nsig;
  b.key_bytes = cb->key_bytes;
  b.sig_bytes = cb->sig_bytes;
  return signed_tx_impl(ctx, &b, &cb->tx, cover);
}

// C5: one device's contiguous shard of both sections, [e0, e1) Ed25519 and
// [c0, c1) ECDSA lanes, streamed in chunks through kStreamStages buffer sets.
// The host enqueues every chunk at once; events do the ordering: a chunk's H2D
// (on s_copy, so PCIe serves the chunks in order and the first one arrives at
// full rate) waits until its stage's previous chunk has finished with the
// buffers; each section's kernels wait for that section's copies. While one
// chunk computes, the next chunks' inputs and the previous chunk's statuses
// cross PCIe, and a chunk's ECDSA kernels (small, the batch inversion
// latency-bound) run beside its Ed25519 ladder on their own stream.
int stream_shard(Device& d, const cordahip_stream_batch* b, uint64_t e0, uint64_t e1, uint64_t c0, uint64_t c1) {
  std::lock_guard<std::mutex> g(d.stream_mu);
  const NodeBind nb(d);
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  const uint64_t ne = e1 - e0, nc = c1 - c0;
  uint64_t chunk = kStreamChunk;  // CORDAHIP_STREAM_CHUNK: smaller chunks for tests of the pipeline itself
  if (const char* v = getenv("CORDAHIP_STREAM_CHUNK")) chunk = std::max<uint64_t>(64, strtoull(v, nullptr, 10));
  // Chunk boundaries over the combined lane count T = ne + nc, each section cut
  // at the same fraction of its length (64-aligned). The first chunks ramp up
  // (chunk/16, chunk/4, then chunk): the GPU starts after a short first copy
  // instead of a full chunk's H2D (~1.2 GB for C5), and PCIe (~4x faster than
  // the kernels per lane) stays ahead while the sizes grow.
  const uint64_t T = ne + nc;
  std::vector<uint64_t> bound(1, 0);  // cumulative combined lanes at chunk ends
  for (int k = 0; bound.back() < T; k++) {
    const uint64_t sz = std::max<uint64_t>(64, k == 0 ? chunk / 16 : k == 1 ? chunk / 4 : chunk);
    bound.push_back(std::min(T, bound.back() + sz));
  }
  const uint64_t nchunks = std::max<size_t>(1, bound.size() - 1);
  auto cut = [&](uint64_t n, uint64_t k) -> uint64_t {  // section offset at the end of chunk k-1
    if (k >= nchunks) return n;
    const uint64_t v = (uint64_t)((__uint128_t)n * bound[k] / (T ? T : 1));
    return std::min(n, v / 64 * 64);
  };
  uint64_t ce = 0, cc = 0;  // largest per-chunk section sizes: the stage buffers
  for (uint64_t k = 0; k < nchunks; k++) {
    ce = std::max(ce, cut(ne, k + 1) - cut(ne, k));
    cc = std::max(cc, cut(nc, k + 1) - cut(nc, k));
  }
  const uint64_t eml = b->ed_msg_len, cml = b->ec_msg_len;
  if (ensure_streams(d) != hipSuccess) return CORDAHIP_ERR_HIP;
  for (StreamStage& st : d.sstage) {
    for (hipEvent_t* pe : {&st.ed_copied, &st.ec_copied, &st.ed_done, &st.ec_done})
      if (!*pe && hipEventCreateWithFlags(pe, hipEventDisableTiming) != hipSuccess) return CORDAHIP_ERR_HIP;
    // a grow replaces buffers: the previous call's work on them is finished
    // (every call synchronises its streams before returning)
    if ((ce && (st.ed_keys.ensure(ce * 32) || st.ed_sigs.ensure(ce * 64) ||
                st.ed_msgs.ensure(std::max<uint64_t>(ce * eml, 16)) || st.ed_status.ensure(ce))) ||
        (cc && (st.ec_scheme.ensure(cc) || st.ec_keys.ensure(cc * 65) || st.ec_key_len.ensure(cc) ||
                st.ec_sigs.ensure(cc * 72) || st.ec_sig_len.ensure(cc) ||
                st.ec_msgs.ensure(std::max<uint64_t>(cc * cml, 16)) || st.ec_status.ensure(cc))))
      return CORDAHIP_ERR_OUT_OF_MEMORY;
  }
  const hipMemcpyKind h2d = hipMemcpyHostToDevice, d2h = hipMemcpyDeviceToHost;
  hipStream_t cs = d.s_copy, xs = d.s_ec;
  // statuses reach pinned caller arrays by kernel stores (a D2H copy queued
  // behind busy compute streams can hold the enqueuing thread for milliseconds,
  // delaying the next chunks' H2D: profiles/r04_q); pageable ones by copies
  uint8_t* map_ed = static_cast<uint8_t*>(host_mapped(b->ed_status));
  uint8_t* map_ec = static_cast<uint8_t*>(host_mapped(b->ec_status));
  hipError_t e = hipSuccess;
  for (uint64_t k = 0; k < nchunks && e == hipSuccess; k++) {
    StreamStage& st = d.sstage[k % kStreamStages];
    // consecutive chunks alternate between s_ed / s_ed2 and the two Ed25519
    // workspace slots: chunk k + 1's prep fills the CUs chunk k's ladder tail
    // leaves idle
    const int slot = (int)(k & 1);
    hipStream_t es = slot ? d.s_ed2 : d.s_ed;
    const uint64_t a = e0 + cut(ne, k), ma = cut(ne, k + 1) - cut(ne, k);
    const uint64_t c = c0 + cut(nc, k), mc = cut(nc, k + 1) - cut(nc, k);
    if (k >= (uint64_t)kStreamStages) {  // the stage's buffers: chunk k-3 must be done with them
      e = hipStreamWaitEvent(cs, st.ed_done, 0);
      e = e ? e : hipStreamWaitEvent(cs, st.ec_done, 0);
    }
    if (ma) {
      e = e ? e : hipMemcpyAsync(st.ed_keys.p, b->ed_keys + a * 32, ma * 32, h2d, cs);
      e = e ? e : hipMemcpyAsync(st.ed_sigs.p, b->ed_sigs + a * 64, ma * 64, h2d, cs);
      if (eml) e = e ? e : hipMemcpyAsync(st.ed_msgs.p, b->ed_msgs + a * eml, ma * eml, h2d, cs);
    }
    e = e ? e : hipEventRecord(st.ed_copied, cs);
    if (mc) {
      e = e ? e : hipMemcpyAsync(st.ec_scheme.p, b->ec_scheme + c, mc, h2d, cs);
      e = e ? e : hipMemcpyAsync(st.ec_keys.p, b->ec_keys + c * 65, mc * 65, h2d, cs);
      e = e ? e : hipMemcpyAsync(st.ec_key_len.p, b->ec_key_len + c, mc, h2d, cs);
      e = e ? e : hipMemcpyAsync(st.ec_sigs.p, b->ec_sigs + c * 72, mc * 72, h2d, cs);
      e = e ? e : hipMemcpyAsync(st.ec_sig_len.p, b->ec_sig_len + c, mc, h2d, cs);
      if (cml) e = e ? e : hipMemcpyAsync(st.ec_msgs.p, b->ec_msgs + c * cml, mc * cml, h2d, cs);
    }
    e = e ? e : hipEventRecord(st.ec_copied, cs);
    e = e ? e : hipStreamWaitEvent(es, st.ed_copied, 0);
    if (ma)
      e = e ? e
            : ed_verify_enqueue(d, st.ed_keys.as<uint8_t>(), st.ed_sigs.as<uint8_t>(), st.ed_msgs.as<uint8_t>(),
                                (uint32_t)eml, ma, nullptr, st.ed_status.as<uint8_t>(), nullptr, 0u, es, slot);
    if (ma && map_ed) e = e ? e : launch_store_to_host(st.ed_status.p, map_ed + a, ma, es);
    else if (ma) e = e ? e : hipMemcpyAsync(b->ed_status + a, st.ed_status.p, ma, d2h, es);
    e = e ? e : hipEventRecord(st.ed_done, es);
    e = e ? e : hipStreamWaitEvent(xs, st.ec_copied, 0);
    if (mc && e == hipSuccess) {
      std::lock_guard<std::mutex> ge(d.ec_mu[0]);
      e = ec_verify_enqueue(d, st.ec_scheme.as<uint8_t>(), st.ec_keys.as<uint8_t>(), st.ec_key_len.as<uint8_t>(),
                            st.ec_sigs.as<uint8_t>(), st.ec_sig_len.as<uint8_t>(), st.ec_msgs.as<uint8_t>(), nullptr,
                            (uint32_t)cml, mc, nullptr, st.ec_status.as<uint8_t>(), nullptr, 0u, xs);
    }
    if (mc && map_ec) e = e ? e : launch_store_to_host(st.ec_status.p, map_ec + c, mc, xs);
    else if (mc) e = e ? e : hipMemcpyAsync(b->ec_status + c, st.ec_status.p, mc, d2h, xs);
    e = e ? e : hipEventRecord(st.ec_done, xs);
  }
  // drain all four streams even after an error, so no queued work outlives the call
  const hipError_t e1s = hipStreamSynchronize(cs), e2s = hipStreamSynchronize(d.s_ed),
                   e2b = hipStreamSynchronize(d.s_ed2), e3s = hipStreamSynchronize(xs);
  if (e != hipSuccess || e1s != hipSuccess || e2s != hipSuccess || e2b != hipSuccess || e3s != hipSuccess)
    return CORDAHIP_ERR_HIP;
  return CORDAHIP_SUCCESS;
}

int stream_verify_impl(cordahip_ctx* ctx, const cordahip_stream_batch* b) {
  if ((b->n_ed && (!b->ed_keys || !b->ed_sigs || !b->ed_status || (b->ed_msg_len && !b->ed_msgs))) ||
      (b->n_ec && (!b->ec_scheme || !b->ec_keys || !b->ec_key_len || !b->ec_sigs || !b->ec_sig_len ||
                   !b->ec_status || (b->ec_msg_len && !b->ec_msgs))))
    return CORDAHIP_ERR_INVALID_ARG;
  const uint64_t nd = ctx->devs.size();
  std::vector<std::future<int>> fs;
  for (uint64_t i = 0; i < nd; i++) {
    uint64_t e0, e1, c0, c1;
    shard_range(b->n_ed, nd, i, 64, e0, e1);
    shard_range(b->n_ec, nd, i, 64, c0, c1);
    if (e0 >= e1 && c0 >= c1) continue;
    Device* d = ctx->devs[i].get();
    fs.push_back(std::async(std::launch::async, [=] { return stream_shard(*d, b, e0, e1, c0, c1); }));
  }
  int rc = CORDAHIP_SUCCESS;
  for (auto& f : fs) {
    const int r = f.get();
    if (r != CORDAHIP_SUCCESS && rc == CORDAHIP_SUCCESS) rc = r;
  }
  return rc;
}

// FilteredTransaction.verify for txs [t0, t1) on one device: K3 hashes the
// filtered leaves, K6 evaluates each partial tree and compares.
int filtered_tx_shard(Device& d, const cordahip_filtered_tx_batch* b, uint64_t t0, uint64_t t1) {
  SetLease lease(d);
  TxSet& S = lease.get();
  const NodeBind nb(d);
  const Activity act(d);
  if (int rc = tx_acquire_host(d, S)) return rc;
  const uint64_t ntx = t1 - t0;
  const uint64_t l0 = b->tx_leaf_off[t0], l1 = b->tx_leaf_off[t1], nleaves = l1 - l0;
  const uint64_t b0 = nleaves ? b->leaf_off[l0] : 0, b1 = nleaves ? b->leaf_off[l1] : 0;
  const uint64_t k0 = b->tx_tok_off[t0], k1 = b->tx_tok_off[t1], ntok = k1 - k0;
  std::vector<uint64_t> loff(nleaves + 1), toff(ntx + 1), koff(ntx + 1);
  for (uint64_t i = 0; i <= nleaves; i++) loff[i] = nleaves ? b->leaf_off[l0 + i] - b0 : 0;
  for (uint64_t i = 0; i <= ntx; i++) {
    toff[i] = b->tx_leaf_off[t0 + i] - l0;
    koff[i] = b->tx_tok_off[t0 + i] - k0;
  }
  TxWork& w = S.tx;
  if (w.leaf_bytes.ensure(std::max<uint64_t>(b1 - b0, 16)) || w.leaf_off.ensure((nleaves + 1) * 8) ||
      w.tx_leaf_off.ensure((ntx + 1) * 8) || w.hashes.ensure(std::max<uint64_t>(nleaves, 1) * 32) ||
      w.tok.ensure(std::max<uint64_t>(ntok, 1)) || w.tok_hash.ensure(std::max<uint64_t>(ntok, 1) * 32) ||
      w.tx_tok_off.ensure((ntx + 1) * 8) || w.root.ensure(ntx * 32) ||
      w.stack.ensure(std::max<uint64_t>(ntok, 1) * 32) || w.tx_status.ensure(ntx))
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  hipStream_t s = d.stream;
  const hipMemcpyKind h2d = hipMemcpyHostToDevice;
  hipError_t e = hipSuccess;
  if (b1 > b0) e = hipMemcpyAsync(w.leaf_bytes.p, b->leaf_bytes + b0, b1 - b0, h2d, s);
  e = e ? e : hipMemcpyAsync(w.leaf_off.p, loff.data(), (nleaves + 1) * 8, h2d, s);
  e = e ? e : hipMemcpyAsync(w.tx_leaf_off.p, toff.data(), (ntx + 1) * 8, h2d, s);
  if (ntok) {
    e = e ? e : hipMemcpyAsync(w.tok.p, b->tok + k0, ntok, h2d, s);
    e = e ? e : hipMemcpyAsync(w.tok_hash.p, b->tok_hash + k0 * 32, ntok * 32, h2d, s);
  }
  e = e ? e : hipMemcpyAsync(w.tx_tok_off.p, koff.data(), (ntx + 1) * 8, h2d, s);
  e = e ? e : hipMemcpyAsync(w.root.p, b->root + t0 * 32, ntx * 32, h2d, s);
  e = e ? e : launch_sha256_leaves(w.leaf_bytes.as<uint8_t>(), w.leaf_off.as<uint64_t>(), nleaves,
                                   w.hashes.as<uint32_t>(), s);
  e = e ? e : launch_pmt_verify(w.hashes.as<uint32_t>(), w.tx_leaf_off.as<uint64_t>(), w.tok.as<uint8_t>(),
                                w.tok_hash.as<uint8_t>(), w.tx_tok_off.as<uint64_t>(), w.root.as<uint8_t>(), ntx,
                                w.stack.as<uint32_t>(), w.tx_status.as<uint8_t>(), s);
  e = e ? e : hipMemcpyAsync(b->tx_status + t0, w.tx_status.p, ntx, hipMemcpyDeviceToHost, s);
  e = e ? e : S.tx_ev.record(s);
  e = e ? e : S.tx_ev.sync();
  if (e != hipSuccess) (void)hipStreamSynchronize(s);
  return hip_err(e);
}

int filtered_tx_impl(cordahip_ctx* ctx, const cordahip_filtered_tx_batch* b) {
  const uint64_t n = b->ntx;
  if (n == 0) return CORDAHIP_SUCCESS;
  if (!b->leaf_off || !b->tx_leaf_off || !b->tx_tok_off || !b->root || !b->tx_status ||
      (!b->tok && b->tx_tok_off[n]) || (!b->tok_hash && b->tx_tok_off[n]))
    return CORDAHIP_ERR_INVALID_ARG;
  if (!check_filtered_batch(PoolPar{*ctx->host}, b)) return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  return for_shards(ctx->devs, n, 1, [&](Device& d, uint64_t t0, uint64_t t1) { return filtered_tx_shard(d, b, t0, t1); });
}

// Typed notary tear-offs [t0, t1) on one device: K21 hashes the StateRef / TimeWindow
// leaves from their rows, K6 evaluates each partial tree over them (notary_stage.hpp).
int notary_tearoff_shard(Device& d, const cordahip_notary_tearoff_batch* b, uint64_t t0, uint64_t t1) {
  SetLease lease(d);
  TxSet& S = lease.get();
  const NodeBind nb(d);
  const Activity act(d);
  if (int rc = tx_acquire_host(d, S)) return rc;
  NotaryStage st(b, t0, t1);
  st.scratch();
  TxWork& w = S.tx;
  if (w.leaf_bytes.ensure(st.pos)) return CORDAHIP_ERR_OUT_OF_MEMORY;
  std::vector<uint8_t> h(st.out_end);
  st.fill(b, h.data());
  uint8_t* dv = w.leaf_bytes.as<uint8_t>();
  hipStream_t s = d.stream;
  hipError_t e = hipMemcpyAsync(dv, h.data(), st.in_bytes, hipMemcpyHostToDevice, s);
  e = e ? e : st.enqueue_verify(dv, b->leaf_hash != nullptr, s);
  e = e ? e : hipMemcpyAsync(h.data() + st.o_vst, dv + st.o_vst, (b->leaf_hash ? st.out_end : st.o_lh) - st.o_vst,
                             hipMemcpyDeviceToHost, s);
  e = e ? e : S.tx_ev.record(s);
  e = e ? e : S.tx_ev.sync();
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    return hip_err(e);
  }
  std::memcpy(b->tx_status + t0, h.data() + st.o_vst, st.ntx);
  if (b->leaf_hash) {
    const uint64_t l0 = NotaryStage::leaves_before(b, t0), l1 = NotaryStage::leaves_before(b, t1);
    std::memcpy(b->leaf_hash + l0 * 32, h.data() + st.o_lh, (l1 - l0) * 32);
  }
  return CORDAHIP_SUCCESS;
}

int notary_tearoff_impl(cordahip_ctx* ctx, const cordahip_notary_tearoff_batch* b) {
  if (!check_notary_tearoff(PoolPar{*ctx->host}, b)) return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  const uint64_t n = b->ntx;
  if (n == 0) return CORDAHIP_SUCCESS;
  if (!notary_pointers_ok(b)) return CORDAHIP_ERR_INVALID_ARG;
  return for_shards(ctx->devs, n, 1,
                    [&](Device& d, uint64_t t0, uint64_t t1) { return notary_tearoff_shard(d, b, t0, t1); });
}

int notary_tearoff_device_impl(cordahip_ctx* ctx, int device, const cordahip_notary_tearoff_batch* b, void* d_tw_from,
                               void* d_tw_until, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d) return CORDAHIP_ERR_INVALID_ARG;
  const int given = (b->tw_flags != nullptr) + (b->tw_from_s != nullptr) + (b->tw_from_nano != nullptr) +
                    (b->tw_until_s != nullptr) + (b->tw_until_nano != nullptr);
  if (given != 0 && given != 5) return CORDAHIP_ERR_INVALID_ARG;
  const uint64_t ntx = b->ntx;
  if (ntx == 0) return CORDAHIP_SUCCESS;
  if (!b->tx_ref_off || !b->tx_tok_off || !b->root || !b->tx_status || !d_tw_from || !d_tw_until ||
      (b->n_refs && !b->refs) || (b->ntok && (!b->tok || !b->tok_hash)) || b->n_refs > (1ull << 56) ||
      ntx > (1ull << 56) || b->ntok > (1ull << 56))
    return CORDAHIP_ERR_INVALID_ARG;
  if (misaligned(b->refs, 4) || misaligned(b->tx_ref_off, 8) || misaligned(b->tx_tok_off, 8) ||
      misaligned(b->tw_from_s, 8) || misaligned(b->tw_until_s, 8) || misaligned(b->tw_from_nano, 4) ||
      misaligned(b->tw_until_nano, 4) || misaligned(b->leaf_hash, 4) || misaligned(d_tw_from, 8) ||
      misaligned(d_tw_until, 8))
    return CORDAHIP_ERR_INVALID_ARG;
  SetLease lease(*d);
  TxSet& S = lease.get();
  TxWork& w = S.tx;
  const uint64_t nl = b->n_refs + ntx, nk = std::max<uint64_t>(b->ntok, 1);
  const NotaryRows R{ntx,          b->n_refs,    b->refs,       b->tx_ref_off,   b->tw_flags,
                     b->tw_from_s, b->tw_from_nano, b->tw_until_s, b->tw_until_nano};
  return device_call(
      *d, hip_stream,
      [&] {
        return S.tx_ev.grow(w.hashes.cap < nl * 32 || w.tx_leaf_off.cap < (ntx + 1) * 8 || w.stack.cap < nk * 32 ||
                                w.pmt_has.cap < ntx,
                            [&] {
                              return w.hashes.ensure(nl * 32) || w.tx_leaf_off.ensure((ntx + 1) * 8) ||
                                             w.stack.ensure(nk * 32) || w.pmt_has.ensure(ntx)
                                         ? hipErrorOutOfMemory
                                         : hipSuccess;
                            });
      },
      [&](hipStream_t s) {
        hipError_t e = S.tx_ev.wait(s);  // the set's previous user is done
        e = e ? e : launch_notary_leaves(R, w.tx_leaf_off.as<uint64_t>(), w.hashes.as<uint32_t>(), b->leaf_hash,
                                         static_cast<int64_t*>(d_tw_from), static_cast<int64_t*>(d_tw_until),
                                         w.pmt_has.as<uint8_t>(), s);
        e = e ? e : launch_pmt_verify(w.hashes.as<uint32_t>(), w.tx_leaf_off.as<uint64_t>(), b->tok, b->tok_hash,
                                      b->tx_tok_off, b->root, ntx, w.stack.as<uint32_t>(), b->tx_status, s,
                                      w.pmt_has.as<uint8_t>());
        return e ? e : S.tx_ev.record(s);
      });
}

// FilteredTransaction build for txs [t0, t1) on one device: K3 hashes the
// leaves, K10 builds each tree and writes its tokens into the caller's slot.
// The shard's slots are the contiguous token range [tx_tok_off[t0], tx_tok_off[t1]),
// which comes back whole (entries past a transaction's tx_ntok are unspecified).
int filtered_build_shard(Device& d, const cordahip_filtered_build_batch* b, uint64_t t0, uint64_t t1) {
  SetLease lease(d);
  TxSet& S = lease.get();
  const NodeBind nb(d);
  const Activity act(d);
  if (int rc = tx_acquire_host(d, S)) return rc;
  const uint64_t ntx = t1 - t0;
  const uint64_t l0 = b->tx_leaf_off[t0], l1 = b->tx_leaf_off[t1], nleaves = l1 - l0;
  const uint64_t b0 = nleaves ? b->leaf_off[l0] : 0, b1 = nleaves ? b->leaf_off[l1] : 0;
  const uint64_t k0 = b->tx_tok_off[t0], k1 = b->tx_tok_off[t1], ntok = k1 - k0;
  std::vector<uint64_t> loff(nleaves + 1), toff(ntx + 1), koff(ntx + 1);
  for (uint64_t i = 0; i <= nleaves; i++) loff[i] = nleaves ? b->leaf_off[l0 + i] - b0 : 0;
  for (uint64_t i = 0; i <= ntx; i++) {
    toff[i] = b->tx_leaf_off[t0 + i] - l0;
    koff[i] = b->tx_tok_off[t0 + i] - k0;
  }
  TxWork& w = S.tx;
  const uint64_t nl1 = std::max<uint64_t>(nleaves, 1);
  if (w.leaf_bytes.ensure(std::max<uint64_t>(b1 - b0, 16)) || w.leaf_off.ensure((nleaves + 1) * 8) ||
      w.tx_leaf_off.ensure((ntx + 1) * 8) || w.hashes.ensure(nl1 * 32) || w.incl.ensure(nl1) ||
      w.pmt_up.ensure(nl1 * 64) || w.pmt_has.ensure(nl1 * 3) || w.tx_tok_off.ensure((ntx + 1) * 8) ||
      w.tok.ensure(std::max<uint64_t>(ntok, 1)) || w.tok_hash.ensure(std::max<uint64_t>(ntok, 1) * 32) ||
      w.txid.ensure(ntx * 32) || w.tx_ntok.ensure(ntx * 8) || w.tx_status.ensure(ntx))
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  hipStream_t s = d.stream;
  const hipMemcpyKind h2d = hipMemcpyHostToDevice, d2h = hipMemcpyDeviceToHost;
  hipError_t e = hipSuccess;
  if (b1 > b0) e = hipMemcpyAsync(w.leaf_bytes.p, b->leaf_bytes + b0, b1 - b0, h2d, s);
  e = e ? e : hipMemcpyAsync(w.leaf_off.p, loff.data(), (nleaves + 1) * 8, h2d, s);
  e = e ? e : hipMemcpyAsync(w.tx_leaf_off.p, toff.data(), (ntx + 1) * 8, h2d, s);
  if (nleaves) e = e ? e : hipMemcpyAsync(w.incl.p, b->include + l0, nleaves, h2d, s);
  e = e ? e : hipMemcpyAsync(w.tx_tok_off.p, koff.data(), (ntx + 1) * 8, h2d, s);
  e = e ? e : launch_sha256_leaves(w.leaf_bytes.as<uint8_t>(), w.leaf_off.as<uint64_t>(), nleaves,
                                   w.hashes.as<uint32_t>(), s);
  e = e ? e : launch_pmt_build(w.hashes.as<uint32_t>(), w.tx_leaf_off.as<uint64_t>(), ntx, w.incl.as<uint8_t>(),
                               w.tx_tok_off.as<uint64_t>(), ntok, w.pmt_up.as<uint32_t>(), w.pmt_has.as<uint8_t>(),
                               w.txid.as<uint8_t>(), w.tok.as<uint8_t>(), w.tok_hash.as<uint8_t>(),
                               w.tx_ntok.as<uint64_t>(), w.tx_status.as<uint8_t>(), s);
  e = e ? e : hipMemcpyAsync(b->txid + t0 * 32, w.txid.p, ntx * 32, d2h, s);
  e = e ? e : hipMemcpyAsync(b->tx_ntok + t0, w.tx_ntok.p, ntx * 8, d2h, s);
  e = e ? e : hipMemcpyAsync(b->tx_status + t0, w.tx_status.p, ntx, d2h, s);
  if (ntok) {
    e = e ? e : hipMemcpyAsync(b->tok + k0, w.tok.p, ntok, d2h, s);
    e = e ? e : hipMemcpyAsync(b->tok_hash + k0 * 32, w.tok_hash.p, ntok * 32, d2h, s);
  }
  e = e ? e : S.tx_ev.record(s);
  e = e ? e : S.tx_ev.sync();
  if (e != hipSuccess) (void)hipStreamSynchronize(s);
  return hip_err(e);
}

int filtered_build_impl(cordahip_ctx* ctx, const cordahip_filtered_build_batch* b) {
  const uint64_t n = b->ntx;
  if (n == 0) return CORDAHIP_SUCCESS;
  if (!b->leaf_off || !b->tx_leaf_off || !b->tx_tok_off || !b->txid || !b->tx_ntok || !b->tx_status)
    return CORDAHIP_ERR_INVALID_ARG;
  if (!check_filtered_build_batch(PoolPar{*ctx->host}, b)) return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  // the offsets are sound: what they span must exist
  const uint64_t l0 = b->tx_leaf_off[0], l1 = b->tx_leaf_off[n];
  if (l0 != l1 && (!b->include || (b->leaf_off[l0] != b->leaf_off[l1] && !b->leaf_bytes))) return CORDAHIP_ERR_INVALID_ARG;
  if (b->tx_tok_off[0] != b->tx_tok_off[n] && (!b->tok || !b->tok_hash)) return CORDAHIP_ERR_INVALID_ARG;
  return for_shards(ctx->devs, n, 1,
                    [&](Device& d, uint64_t t0, uint64_t t1) { return filtered_build_shard(d, b, t0, t1); });
}

}  // namespace

extern "C" {

uint32_t cordahip_abi_version(void) { return CORDAHIP_ABI_VERSION; }

const char* cordahip_strerror(int code) {
  switch (code) {
    case CORDAHIP_SUCCESS: return "success";
    case CORDAHIP_ERR_INVALID_ARG: return "invalid argument";
    case CORDAHIP_ERR_HIP: return "HIP runtime error";
    case CORDAHIP_ERR_NO_DEVICE: return "no usable HIP device";
    case CORDAHIP_ERR_OUT_OF_MEMORY: return "out of device memory";
    case CORDAHIP_ERR_TIMEOUT: return "timed out";
    case CORDAHIP_ERR_UNKNOWN_TICKET: return "unknown ticket";
    case CORDAHIP_ERR_NOT_IMPLEMENTED: return "not implemented on the GPU path";
    case CORDAHIP_ERR_LOG_FULL: return "commit log full (reserve a larger capacity)";
    default: return "unknown error";
  }
}

void cordahip_shard_range(uint64_t n, uint32_t nshards, uint32_t shard, uint64_t align, uint64_t* lo, uint64_t* hi) {
  uint64_t a, b;
  shard_range(n, nshards, shard, align, a, b);
  if (lo) *lo = a;
  if (hi) *hi = b;
}


int cordahip_device_count(const cordahip_ctx* ctx) { return ctx ? (int)ctx->devs.size() : 0; }

int cordahip_device_mem(cordahip_ctx* ctx, int device, uint64_t* in_use, uint64_t* peak, uint64_t* budget) {
  Device* d = dev_at(ctx, device);
  if (!d) return CORDAHIP_ERR_INVALID_ARG;
  const MemAcct& m = mem_acct(d->id);
  if (in_use) *in_use = m.in_use.load();
  if (peak) *peak = m.peak.load();
  if (budget) *budget = d->mem_budget;
  return CORDAHIP_SUCCESS;
}

int cordahip_trim(cordahip_ctx* ctx) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] {
    for (auto& d : ctx->devs) trim_device(*d);
    return (int)CORDAHIP_SUCCESS;
  });
}

int cordahip_alloc_pinned(cordahip_ctx* ctx, size_t bytes, void** host) {
  if (!ctx || !host) return CORDAHIP_ERR_INVALID_ARG;
  return hipHostMalloc(host, bytes, hipHostMallocPortable) == hipSuccess ? CORDAHIP_SUCCESS
                                                                          : CORDAHIP_ERR_OUT_OF_MEMORY;
}

int cordahip_free_pinned(cordahip_ctx* ctx, void* host) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return hip_err(hipHostFree(host));
}

int cordahip_sig_verify(cordahip_ctx* ctx, const cordahip_sig_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return sig_verify_impl(ctx, batch); });
}

int cordahip_sig_submit(cordahip_ctx* ctx, const cordahip_sig_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, sig_verify_impl, batch);
}

int cordahip_tx_submit(cordahip_ctx* ctx, const cordahip_signed_tx_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, [](cordahip_ctx* c, const cordahip_signed_tx_batch* b) { return signed_tx_impl(c, b); },
                batch);
}

int cordahip_txcomp_submit(cordahip_ctx* ctx, const cordahip_signed_txcomp_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket,
                [](cordahip_ctx* c, const cordahip_signed_txcomp_batch* b) { return signed_txcomp_impl(c, b); }, batch);
}

int cordahip_signed_txcomp_verify(cordahip_ctx* ctx, const cordahip_signed_txcomp_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return signed_txcomp_impl(ctx, batch); });
}

int cordahip_signed_tx_verify_covered(cordahip_ctx* ctx, const cordahip_signed_tx_batch* batch,
                                      const cordahip_cover* cover) {
  if (!ctx || !batch || !cover) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return signed_tx_impl(ctx, batch, nullptr, cover); });
}

int cordahip_tx_submit_covered(cordahip_ctx* ctx, const cordahip_signed_tx_batch* batch, const cordahip_cover* cover,
                               uint64_t* ticket) {
  return submit(ctx, ticket, [](cordahip_ctx* c, const cordahip_signed_tx_batch* b, const cordahip_cover* v) {
    return signed_tx_impl(c, b, nullptr, v);
  }, batch, cover);
}

int cordahip_signed_txcomp_verify_covered(cordahip_ctx* ctx, const cordahip_signed_txcomp_batch* batch,
                                          const cordahip_cover* cover) {
  if (!ctx || !batch || !cover) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return signed_txcomp_impl(ctx, batch, cover); });
}

int cordahip_txcomp_submit_covered(cordahip_ctx* ctx, const cordahip_signed_txcomp_batch* batch,
                                   const cordahip_cover* cover, uint64_t* ticket) {
  return submit(ctx, ticket, [](cordahip_ctx* c, const cordahip_signed_txcomp_batch* b, const cordahip_cover* v) {
    return signed_txcomp_impl(c, b, v);
  }, batch, cover);
}

int cordahip_txid_submit(cordahip_ctx* ctx, const cordahip_txid_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, tx_ids_impl, batch);
}

int cordahip_filtered_tx_submit(cordahip_ctx* ctx, const cordahip_filtered_tx_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, filtered_tx_impl, batch);
}

// a ticket's job (nullptr: unknown, or already waited for)
static std::shared_ptr<JobState> job_of(cordahip_ctx* ctx, uint64_t ticket) {
  std::lock_guard<std::mutex> g(ctx->mu);
  auto it = ctx->jobs.find(ticket);
  return it == ctx->jobs.end() ? nullptr : it->second;
}

int cordahip_wait(cordahip_ctx* ctx, uint64_t ticket, int64_t timeout_ns) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  const std::shared_ptr<JobState> st = job_of(ctx, ticket);
  if (!st) return CORDAHIP_ERR_UNKNOWN_TICKET;
  int rc;
  {
    std::unique_lock<std::mutex> g(st->m);
    if (timeout_ns < 0) st->cv.wait(g, [&] { return st->done; });
    else if (!st->cv.wait_for(g, std::chrono::nanoseconds(timeout_ns), [&] { return st->done; }))
      return CORDAHIP_ERR_TIMEOUT;
    rc = st->rc;
  }
  std::lock_guard<std::mutex> g(ctx->mu);
  ctx->jobs.erase(ticket);  // released: the ticket is single-use
  return rc;
}

int cordahip_poll(cordahip_ctx* ctx, uint64_t ticket) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  const std::shared_ptr<JobState> st = job_of(ctx, ticket);
  if (!st) return CORDAHIP_ERR_UNKNOWN_TICKET;
  std::lock_guard<std::mutex> g(st->m);
  return st->done ? 1 : 0;
}

int cordahip_ed25519_verify_device(cordahip_ctx* ctx, int device, const void* d_keys, const void* d_sigs,
                                   const void* d_msgs, uint32_t msg_len, uint64_t n, void* d_status,
                                   void* d_verdict, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (!d_keys && n) || (!d_sigs && n) || (!d_status && n)) return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_keys) | reinterpret_cast<uintptr_t>(d_sigs)) & 15)
    return CORDAHIP_ERR_INVALID_ARG;
  if (msg_len == 32 && (reinterpret_cast<uintptr_t>(d_msgs) & 15)) return CORDAHIP_ERR_INVALID_ARG;
  return device_call(*d, hip_stream, [&](hipStream_t s) {
    return ed_verify_enqueue(*d, static_cast<const uint8_t*>(d_keys), static_cast<const uint8_t*>(d_sigs),
                             static_cast<const uint8_t*>(d_msgs), msg_len, n, nullptr, static_cast<uint8_t*>(d_status),
                             static_cast<unsigned long long*>(d_verdict), 0u, s);
  });
}

int cordahip_ecdsa_verify_device(cordahip_ctx* ctx, int device, const void* d_scheme, const void* d_keys,
                                 const void* d_key_len, const void* d_sigs, const void* d_sig_len, const void* d_msgs,
                                 uint32_t msg_len, uint64_t n, void* d_status, void* d_verdict, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (n && (!d_scheme || !d_keys || !d_key_len || !d_sigs || !d_sig_len || !d_status || (msg_len && !d_msgs))))
    return CORDAHIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(d->ec_mu[0]);
  return device_call(*d, hip_stream, [&](hipStream_t s) {
    return ec_verify_enqueue(*d, static_cast<const uint8_t*>(d_scheme), static_cast<const uint8_t*>(d_keys),
                             static_cast<const uint8_t*>(d_key_len), static_cast<const uint8_t*>(d_sigs),
                             static_cast<const uint8_t*>(d_sig_len), static_cast<const uint8_t*>(d_msgs), nullptr,
                             msg_len, n, nullptr, static_cast<uint8_t*>(d_status),
                             static_cast<unsigned long long*>(d_verdict), 0u, s);
  });
}

int cordahip_rsa_public_op_device(cordahip_ctx* ctx, int device, const void* d_mod, const void* d_exp,
                                  const void* d_in, uint32_t mod_words, uint64_t n, void* d_out, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (mod_words != 64 && mod_words != 96 && mod_words != 128) || (n && (!d_mod || !d_exp || !d_in || !d_out)))
    return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_mod) | reinterpret_cast<uintptr_t>(d_exp) | reinterpret_cast<uintptr_t>(d_in) |
       reinterpret_cast<uintptr_t>(d_out)) & 3)
    return CORDAHIP_ERR_INVALID_ARG;
  return device_call(*d, hip_stream, [&](hipStream_t s) {
    return launch_rsa_public_op(static_cast<const uint32_t*>(d_mod), static_cast<const uint32_t*>(d_exp),
                                static_cast<const uint32_t*>(d_in), mod_words, n, static_cast<uint32_t*>(d_out), s);
  });
}

int cordahip_rsa_pss_verify_device(cordahip_ctx* ctx, int device, const void* d_mod, const void* d_exp,
                                   const void* d_sigs, const void* d_sig_len, const void* d_msgs, uint32_t msg_len,
                                   uint32_t mod_words, uint64_t n, void* d_status, void* d_verdict, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (mod_words != 64 && mod_words != 96 && mod_words != 128) ||
      (n && (!d_mod || !d_exp || !d_sigs || !d_sig_len || !d_status || (msg_len && !d_msgs))))
    return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_mod) | reinterpret_cast<uintptr_t>(d_exp)) & 3 ||
      reinterpret_cast<uintptr_t>(d_sig_len) & 1)
    return CORDAHIP_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> g(d->rsa_mu);
  return device_call(*d, hip_stream, [&](hipStream_t s) {
    return rsa_verify_enqueue(*d, static_cast<const uint32_t*>(d_mod), static_cast<const uint32_t*>(d_exp),
                              static_cast<const uint8_t*>(d_sigs), static_cast<const uint16_t*>(d_sig_len),
                              static_cast<const uint8_t*>(d_msgs), nullptr, msg_len, mod_words, n, nullptr,
                              static_cast<uint8_t*>(d_status), static_cast<unsigned long long*>(d_verdict), 0u, s);
  });
}

// K23: the generic batch resident in device memory (runtime.cpp sig_device_enqueue)
int cordahip_sig_verify_device(cordahip_ctx* ctx, int device, const void* d_scheme, const void* d_key,
                               const void* d_key_off, uint64_t key_bytes, const void* d_sig, const void* d_sig_off,
                               uint64_t sig_bytes, const void* d_msgs, uint32_t msg_len, const void* d_msg_row,
                               uint64_t msg_rows, uint64_t n, uint32_t flags, void* d_status, void* d_verdict,
                               void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || n >= sigpack::kMaxLanes || (flags & ~(CORDAHIP_FLAG_IS_VALID | CORDAHIP_FLAG_RSA_ON_DEVICE)))
    return CORDAHIP_ERR_INVALID_ARG;
  if (n && (!d_scheme || !d_key_off || !d_sig_off || !d_status || (key_bytes && !d_key) || (sig_bytes && !d_sig) ||
            (msg_len && msg_rows && !d_msgs)))
    return CORDAHIP_ERR_INVALID_ARG;
  if (misaligned(d_key_off, 8) || misaligned(d_sig_off, 8) || misaligned(d_msg_row, 4) || misaligned(d_verdict, 8))
    return CORDAHIP_ERR_INVALID_ARG;
  sigpack::In in{};
  in.scheme = ptr<uint8_t>(d_scheme);
  in.key = ptr<uint8_t>(d_key);
  in.key_off = ptr<uint64_t>(d_key_off);
  in.key_bytes = key_bytes;
  in.sig = ptr<uint8_t>(d_sig);
  in.sig_off = ptr<uint64_t>(d_sig_off);
  in.sig_bytes = sig_bytes;
  in.msg_row = ptr<uint32_t>(d_msg_row);
  in.msg_rows = msg_rows;
  in.msg_len = msg_len;
  in.n = n;
  in.do_verify = (flags & CORDAHIP_FLAG_IS_VALID) ? 0u : 1u;
  in.rsa_on = (flags & CORDAHIP_FLAG_RSA_ON_DEVICE) ? 1u : 0u;
  return guarded([&] {
    return device_call(*d, hip_stream, [&](hipStream_t s) {
      return sig_device_enqueue(*d, in, ptr<uint8_t>(d_msgs), ptr<uint8_t>(d_status),
                                ptr<unsigned long long>(d_verdict), s);
    });
  });
}

int cordahip_set_rsa_on_device(cordahip_ctx* ctx, uint32_t on) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  ctx->rsa_on_device.store(on ? 1u : 0u);
  return CORDAHIP_SUCCESS;
}

int cordahip_tx_cover_device(cordahip_ctx* ctx, int device, uint64_t ntx, void* d_tx_status,
                             const void* d_tx_sig_off, const void* d_sig_scheme, const void* d_sig_key,
                             const void* d_sig_key_off, const cordahip_cover* cover, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || !cover) return CORDAHIP_ERR_INVALID_ARG;
  if (ntx && (!d_tx_status || !d_tx_sig_off || !cover->tx_req_off || !cover->first_missing))
    return CORDAHIP_ERR_INVALID_ARG;
  if (ntx && cover->nreq && (!cover->req_tok_off || !cover->req_status || (cover->ntok && !cover->tok)))
    return CORDAHIP_ERR_INVALID_ARG;
  if (ntx && cover->nckey && (!cover->ckey_scheme || !cover->ckey_off || (cover->ckey_bytes && !cover->ckey)))
    return CORDAHIP_ERR_INVALID_ARG;
  if (!d_sig_key_off && (reinterpret_cast<uintptr_t>(d_sig_key) & 15)) return CORDAHIP_ERR_INVALID_ARG;  // dense rows
  return guarded([&]() -> int {
    // the trees' evaluation stacks, one 8-byte slot per token (shared scratch:
    // cover_mu orders the enqueues, cover_ev fences its reuse across streams)
    std::lock_guard<std::mutex> g(d->cover_mu);
    const uint64_t need = std::max<uint64_t>(cover->ntok, 1) * 8;
    return device_call(
        *d, hip_stream,
        [&] {
          return d->cover_ev.grow(d->cover_stack.cap < need,
                                  [&] { return d->cover_stack.ensure(need) ? hipErrorOutOfMemory : hipSuccess; });
        },
        [&](hipStream_t s) {
          hipError_t e = d->cover_ev.wait(s);  // the previous user of the scratch is done
          e = e ? e
                : launch_tx_cover(*cover, ntx, static_cast<uint8_t*>(d_tx_status),
                                  static_cast<const uint64_t*>(d_tx_sig_off), static_cast<const uint8_t*>(d_sig_scheme),
                                  static_cast<const uint8_t*>(d_sig_key), static_cast<const uint64_t*>(d_sig_key_off),
                                  d->cover_stack.as<uint64_t>(), s);
          return e ? e : d->cover_ev.record(s);
        });
  });
}

int cordahip_txcomp_inputs_device(cordahip_ctx* ctx, int device, const void* d_items, uint64_t n_items,
                                  const void* d_payload, uint64_t payload_len, const void* d_tx_item_off, uint64_t ntx,
                                  const void* d_tx_status, void* d_refs, uint64_t ref_cap, void* d_tx_ref_off,
                                  void* d_tw_from, void* d_tw_until, void* d_gate, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || n_items >= 0x7fffffffull) return CORDAHIP_ERR_INVALID_ARG;
  if (ntx && (!d_tx_item_off || !d_tx_ref_off || !d_tw_from || !d_tw_until || !d_gate || (n_items && !d_items) ||
              (ref_cap && !d_refs) || (payload_len && !d_payload)))
    return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_tx_item_off) | reinterpret_cast<uintptr_t>(d_tx_ref_off) |
       reinterpret_cast<uintptr_t>(d_tw_from) | reinterpret_cast<uintptr_t>(d_tw_until) |
       reinterpret_cast<uintptr_t>(d_items)) & 7 ||
      reinterpret_cast<uintptr_t>(d_refs) & 3)
    return CORDAHIP_ERR_INVALID_ARG;
  return device_call(*d, hip_stream, [&](hipStream_t s) {
    return launch_txcomp_inputs(static_cast<const cordahip_kryo_item*>(d_items), n_items,
                                static_cast<const uint8_t*>(d_payload), payload_len,
                                static_cast<const uint64_t*>(d_tx_item_off), ntx,
                                static_cast<const uint8_t*>(d_tx_status), static_cast<uint32_t*>(d_refs), ref_cap,
                                static_cast<uint64_t*>(d_tx_ref_off), static_cast<int64_t*>(d_tw_from),
                                static_cast<int64_t*>(d_tw_until), static_cast<uint8_t*>(d_gate), s);
  });
}

double cordahip_last_kernel_ms(cordahip_ctx* ctx, int device) {
  Device* d = dev_at(ctx, device);
  if (!d) return -1.0;
  auto it = tl_last_call.find(d->uid);
  if (it == tl_last_call.end()) return -1.0;
  const TimedCall& tc = d->ring[it->second.first];
  {
    std::lock_guard<std::mutex> g(d->tmu);
    if (tc.gen != it->second.second) return -1.0;  // the slot was reused: > kTimingRing calls since
  }
  if (hipEventSynchronize(tc.b) != hipSuccess) return -1.0;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, tc.a, tc.b) != hipSuccess) return -1.0;
  {
    // a concurrent timed_begin may have re-recorded the slot's events between
    // the check above and the read: then ms mixes two calls, so report none
    std::lock_guard<std::mutex> g(d->tmu);
    if (tc.gen != it->second.second) return -1.0;
  }
  return ms;
}

int cordahip_ed25519_verify_host(cordahip_ctx* ctx, const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs,
                                 uint32_t msg_len, uint64_t n, uint8_t* status, uint64_t* verdict) {
  if (!ctx || (n && (!keys || !sigs || !status || (msg_len && !msgs)))) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return ed25519_dense_host(ctx, keys, sigs, msgs, msg_len, n, status, verdict); });
}

int cordahip_filtered_tx_verify(cordahip_ctx* ctx, const cordahip_filtered_tx_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return filtered_tx_impl(ctx, batch); });
}

int cordahip_notary_tearoff_verify(cordahip_ctx* ctx, const cordahip_notary_tearoff_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return notary_tearoff_impl(ctx, batch); });
}

int cordahip_notary_tearoff_submit(cordahip_ctx* ctx, const cordahip_notary_tearoff_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, notary_tearoff_impl, batch);
}

int cordahip_notary_tearoff_device(cordahip_ctx* ctx, int device, const cordahip_notary_tearoff_batch* d_batch,
                                   void* d_tw_from, void* d_tw_until, void* hip_stream) {
  if (!ctx || !d_batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return notary_tearoff_device_impl(ctx, device, d_batch, d_tw_from, d_tw_until, hip_stream); });
}

int cordahip_filtered_tx_build(cordahip_ctx* ctx, const cordahip_filtered_build_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return filtered_build_impl(ctx, batch); });
}

int cordahip_filtered_tx_build_submit(cordahip_ctx* ctx, const cordahip_filtered_build_batch* batch,
                                      uint64_t* ticket) {
  return submit(ctx, ticket, filtered_build_impl, batch);
}

int cordahip_filtered_tx_build_device(cordahip_ctx* ctx, int device, const void* d_leaf_bytes,
                                      const void* d_leaf_off, uint64_t nleaves, const void* d_tx_leaf_off,
                                      uint64_t ntx, const void* d_include, const void* d_tx_tok_off, uint64_t ntok,
                                      void* d_txid, void* d_tok, void* d_tok_hash, void* d_tx_ntok,
                                      void* d_tx_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (ntx && (!d_leaf_off || !d_tx_leaf_off || !d_tx_tok_off || !d_txid || !d_tx_ntok || !d_tx_status)) ||
      (ntx && nleaves && !d_include) || (ntx && ntok && (!d_tok || !d_tok_hash)))
    return CORDAHIP_ERR_INVALID_ARG;
  if (nleaves > (1ull << 56)) return CORDAHIP_ERR_INVALID_ARG;  // the workspace sizes below stay in 64 bits
  // a buffer set for the enqueue: its leaf hashes and tree levels, fenced by its
  // event until these kernels finish (the next holder waits on it)
  SetLease lease(*d);
  TxSet& S = lease.get();
  TxWork& w = S.tx;
  const uint64_t nl1 = std::max<uint64_t>(nleaves, 1);
  return device_call(
      *d, hip_stream,
      [&] {
        return S.tx_ev.grow(w.hashes.cap < nl1 * 32 || w.pmt_up.cap < nl1 * 64 || w.pmt_has.cap < nl1 * 3, [&] {
          return w.hashes.ensure(nl1 * 32) || w.pmt_up.ensure(nl1 * 64) || w.pmt_has.ensure(nl1 * 3)
                     ? hipErrorOutOfMemory
                     : hipSuccess;
        });
      },
      [&](hipStream_t s) {
        hipError_t e = S.tx_ev.wait(s);  // the set's previous user is done
        e = e ? e : launch_sha256_leaves(static_cast<const uint8_t*>(d_leaf_bytes),
                                         static_cast<const uint64_t*>(d_leaf_off), nleaves, w.hashes.as<uint32_t>(), s);
        e = e ? e : launch_pmt_build(w.hashes.as<uint32_t>(), static_cast<const uint64_t*>(d_tx_leaf_off), ntx,
                                     static_cast<const uint8_t*>(d_include), static_cast<const uint64_t*>(d_tx_tok_off),
                                     ntok, w.pmt_up.as<uint32_t>(), w.pmt_has.as<uint8_t>(),
                                     static_cast<uint8_t*>(d_txid), static_cast<uint8_t*>(d_tok),
                                     static_cast<uint8_t*>(d_tok_hash), static_cast<uint64_t*>(d_tx_ntok),
                                     static_cast<uint8_t*>(d_tx_status), s);
        return e ? e : S.tx_ev.record(s);
      });
}

int cordahip_stream_verify(cordahip_ctx* ctx, const cordahip_stream_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return stream_verify_impl(ctx, batch); });
}

int cordahip_ed25519_sign_device(cordahip_ctx* ctx, int device, const void* d_seeds, const void* d_msgs,
                                 uint32_t msg_len, uint64_t n, void* d_pubs, void* d_sigs, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (n && (!d_seeds || !d_pubs || !d_sigs))) return CORDAHIP_ERR_INVALID_ARG;
  if (hipSetDevice(d->id) != hipSuccess) return CORDAHIP_ERR_HIP;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);  // NULL = the device's null stream
  return hip_err(launch_ed25519_sign(static_cast<const uint8_t*>(d_seeds), static_cast<const uint8_t*>(d_msgs),
                                     msg_len, n, d->btab.as<uint32_t>(), static_cast<uint8_t*>(d_pubs),
                                     static_cast<uint8_t*>(d_sigs), s));
}

int cordahip_ecdsa_sign_device(cordahip_ctx* ctx, int device, const void* d_scheme, const void* d_seeds,
                               const void* d_msgs, uint32_t msg_len, uint64_t n, void* d_keys, void* d_key_len,
                               void* d_sigs, void* d_sig_len, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (n && (!d_scheme || !d_seeds || !d_keys || !d_key_len || !d_sigs || !d_sig_len || (msg_len && !d_msgs))))
    return CORDAHIP_ERR_INVALID_ARG;
  if (hipSetDevice(d->id) != hipSuccess) return CORDAHIP_ERR_HIP;
  return hip_err(launch_ecdsa_sign(static_cast<const uint8_t*>(d_scheme), static_cast<const uint8_t*>(d_seeds),
                                   static_cast<const uint8_t*>(d_msgs), msg_len, n, d->gtab_k1.as<uint32_t>(), d->gtab_r1.as<uint32_t>(),
                                   static_cast<uint8_t*>(d_keys), static_cast<uint8_t*>(d_key_len),
                                   static_cast<uint8_t*>(d_sigs), static_cast<uint8_t*>(d_sig_len),
                                   static_cast<hipStream_t>(hip_stream)));
}

int cordahip_tx_ids(cordahip_ctx* ctx, const cordahip_txid_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return tx_ids_impl(ctx, batch); });
}

int cordahip_signed_tx_verify(cordahip_ctx* ctx, const cordahip_signed_tx_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return signed_tx_impl(ctx, batch); });
}

int cordahip_signed_tx_verify_ed25519_device(cordahip_ctx* ctx, int device, const void* d_leaf_bytes,
                                             const void* d_leaf_off, uint64_t nleaves, const void* d_tx_leaf_off,
                                             uint64_t ntx, const void* d_tx_sig_off, const void* d_keys,
                                             const void* d_sigs, uint64_t nsig, void* d_txid, void* d_tx_status,
                                             void* d_first_bad, void* d_sig_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (ntx && (!d_leaf_off || !d_tx_leaf_off || !d_tx_sig_off || !d_txid || !d_tx_status || !d_first_bad)) ||
      (nsig && (!d_keys || !d_sigs || !d_sig_status)))
    return CORDAHIP_ERR_INVALID_ARG;
  // a buffer set for the enqueue; its event then fences the set's hashes / msgs
  // until these kernels finish (the next holder waits on it)
  SetLease lease(*d);
  TxSet& S = lease.get();
  TxWork& w = S.tx;
  const DeviceSignedTx c{*d, S, ntx, d_tx_sig_off, d_keys, d_sigs, nsig, d_txid, d_tx_status, d_first_bad, d_sig_status};
  return device_call(
      *d, hip_stream, [&] { return c.prepare(nleaves, false); },
      [&](hipStream_t s) {
        hipStream_t x = nullptr;
        hipError_t e = c.fork(s, x);
        e = e ? e : launch_sha256_leaves(static_cast<const uint8_t*>(d_leaf_bytes),
                                         static_cast<const uint64_t*>(d_leaf_off), nleaves, w.hashes.as<uint32_t>(), x);
        e = e ? e : launch_merkle_root(w.hashes.as<uint32_t>(), static_cast<const uint64_t*>(d_tx_leaf_off), ntx,
                                       static_cast<uint8_t*>(d_txid), static_cast<uint8_t*>(d_tx_status), x);
        return e ? e : c.join_and_verify(s, x);
      });
}

// the signatures of a mixed-scheme device signed-tx call as the packer's input, or false
static bool mixed_sigs(cordahip_ctx* ctx, const void* d_scheme, const void* d_key, const void* d_key_off,
                       uint64_t key_bytes, const void* d_sig, const void* d_sig_off, uint64_t sig_bytes, uint64_t nsig,
                       const void* d_sig_status, sigpack::In& in) {
  if (nsig >= sigpack::kMaxLanes) return false;
  if (nsig && (!d_scheme || !d_key_off || !d_sig_off || !d_sig_status || (key_bytes && !d_key) || (sig_bytes && !d_sig)))
    return false;
  if (misaligned(d_key_off, 8) || misaligned(d_sig_off, 8)) return false;
  in = sigpack::In{};
  in.scheme = ptr<uint8_t>(d_scheme);
  in.key = ptr<uint8_t>(d_key);
  in.key_off = ptr<uint64_t>(d_key_off);
  in.key_bytes = key_bytes;
  in.sig = ptr<uint8_t>(d_sig);
  in.sig_off = ptr<uint64_t>(d_sig_off);
  in.sig_bytes = sig_bytes;
  in.n = nsig;
  in.do_verify = 1;  // checkSignaturesAreValid: doVerify rules
  in.rsa_on = ctx->rsa_on_device.load() ? 1u : 0u;
  return true;
}

int cordahip_signed_tx_verify_device(cordahip_ctx* ctx, int device, const void* d_leaf_bytes, const void* d_leaf_off,
                                     uint64_t nleaves, const void* d_tx_leaf_off, uint64_t ntx,
                                     const void* d_tx_sig_off, const void* d_scheme, const void* d_key,
                                     const void* d_key_off, uint64_t key_bytes, const void* d_sig,
                                     const void* d_sig_off, uint64_t sig_bytes, uint64_t nsig, void* d_txid,
                                     void* d_tx_status, void* d_first_bad, void* d_sig_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  sigpack::In in;
  if (!d || (ntx && (!d_leaf_off || !d_tx_leaf_off || !d_tx_sig_off || !d_txid || !d_tx_status || !d_first_bad)) ||
      !mixed_sigs(ctx, d_scheme, d_key, d_key_off, key_bytes, d_sig, d_sig_off, sig_bytes, nsig, d_sig_status, in))
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    SetLease lease(*d);
    TxSet& S = lease.get();
    TxWork& w = S.tx;
    const DeviceSignedTx c{*d,   S,      ntx,         d_tx_sig_off, nullptr,      nullptr,
                           nsig, d_txid, d_tx_status, d_first_bad,  d_sig_status, &in};
    return device_call(
        *d, hip_stream, [&] { return c.prepare(nleaves, false); },
        [&](hipStream_t s) {
          hipStream_t x = nullptr;
          hipError_t e = c.fork(s, x);
          e = e ? e : launch_sha256_leaves(static_cast<const uint8_t*>(d_leaf_bytes),
                                           static_cast<const uint64_t*>(d_leaf_off), nleaves, w.hashes.as<uint32_t>(), x);
          e = e ? e : launch_merkle_root(w.hashes.as<uint32_t>(), static_cast<const uint64_t*>(d_tx_leaf_off), ntx,
                                         static_cast<uint8_t*>(d_txid), static_cast<uint8_t*>(d_tx_status), x);
          return e ? e : c.join_and_verify(s, x);
        });
  });
}

int cordahip_kryo_encode_device(cordahip_ctx* ctx, int device, const void* d_items, uint64_t n, uint32_t group,
                                void* d_out, uint64_t cap, void* d_off, void* d_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || !d_off || (n && (!d_items || !d_status))) return CORDAHIP_ERR_INVALID_ARG;
  if (n >= (1ull << 31) - 1) return CORDAHIP_ERR_INVALID_ARG;  // the scan counts items in an int
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(d->kryo_mu);
    return device_call(
        *d, hip_stream,
        [&] {
          size_t temp_bytes = 0;
          const hipError_t e = kryo_scan_bytes(temp_bytes, n + 1, static_cast<hipStream_t>(hip_stream));
          return e ? e : kryo_scratch_ensure(*d, n, std::max<size_t>(temp_bytes, 16));
        },
        [&](hipStream_t s) {
          uint32_t* slots = d->kryo_items.as<uint32_t>();
          hipError_t e = d->kryo_ev.wait(s);  // the previous user of the scratch is done
          e = e ? e : kryo_state_ready(*d, s);
          e = e ? e
                : launch_kryo_encode(static_cast<const cordahip_kryo_item*>(d_items), nullptr, 0, n, group,
                                     d->kryo_fixed.as<uint8_t>(), slots, slots + n, d->kryo_sizes.as<uint64_t>(),
                                     static_cast<uint64_t*>(d_off), static_cast<uint8_t*>(d_out), d_out ? cap : 0,
                                     static_cast<uint8_t*>(d_status), d->kryo_ws.as<uint8_t>(), kKryoDirectWriters,
                                     d->kryo_temp.p, d->kryo_temp.cap, s);
          e = e ? e : kryo_usage_report(*d, nullptr, s);
          return e ? e : d->kryo_ev.record(s);
        });
  });
}

int cordahip_signed_txcomp_verify_ed25519_device(cordahip_ctx* ctx, int device, const void* d_items,
                                                 uint64_t n_items, uint32_t group, const void* d_payload,
                                                 uint64_t payload_len, const void* d_tx_item_off, uint64_t ntx,
                                                 const void* d_tx_sig_off, const void* d_keys, const void* d_sigs,
                                                 uint64_t nsig, void* d_txid, void* d_tx_status, void* d_first_bad,
                                                 void* d_sig_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (ntx && (!d_tx_item_off || !d_tx_sig_off || !d_txid || !d_tx_status || !d_first_bad)) ||
      (n_items && !d_items) || (payload_len && !d_payload) || (nsig && (!d_keys || !d_sigs || !d_sig_status)))
    return CORDAHIP_ERR_INVALID_ARG;
  if (n_items >= (1ull << 31) - 1) return CORDAHIP_ERR_INVALID_ARG;  // the encoder's item slots and lists are 32-bit
  if ((reinterpret_cast<uintptr_t>(d_keys) | reinterpret_cast<uintptr_t>(d_sigs)) & 15) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    // a buffer set for the enqueue (its hashes, messages and component statuses, fenced
    // by its event until these kernels finish) and the encoder's scratch (kryo_mu, kryo_ev)
    SetLease lease(*d);
    TxSet& S = lease.get();
    std::lock_guard<std::mutex> gk(d->kryo_mu);
    TxWork& w = S.tx;
    const DeviceSignedTx c{*d, S, ntx, d_tx_sig_off, d_keys, d_sigs, nsig, d_txid, d_tx_status, d_first_bad, d_sig_status};
    return device_call(
        *d, hip_stream,
        [&] {
          const hipError_t e = c.prepare(n_items, true);
          return e ? e : kryo_scratch_ensure(*d, n_items, 0);
        },
        [&](hipStream_t s) {
          uint32_t* slots = d->kryo_items.as<uint32_t>();
          hipStream_t x = nullptr;
          hipError_t e = d->kryo_ev.wait(s);  // the previous users of the encoder's scratch are done
          e = e ? e : c.fork(s, x);
          e = e ? e : kryo_state_ready(*d, x);
          // leaf hashes from the templates (misses impossible: new shapes are built, the rest
          // hashed by the direct encoder), then the ids, with a rejected component making its
          // transaction CORDAHIP_TX_BAD_COMPONENT
          e = e ? e
                : launch_kryo_hash_chain(static_cast<const cordahip_kryo_item*>(d_items),
                                         static_cast<const uint8_t*>(d_payload), payload_len, n_items, group,
                                         d->kryo_fixed.as<uint8_t>(), slots, slots + n_items,
                                         d->kryo_sizes.as<uint64_t>(), w.comp_status.as<uint8_t>(),
                                         w.hashes.as<uint32_t>(), d->kryo_ws.as<uint8_t>(), kKryoDirectWriters, x);
          e = e ? e : kryo_usage_report(*d, nullptr, x);
          e = e ? e : d->kryo_ev.record(x);
          e = e ? e : launch_merkle_root(w.hashes.as<uint32_t>(), static_cast<const uint64_t*>(d_tx_item_off), ntx,
                                         static_cast<uint8_t*>(d_txid), static_cast<uint8_t*>(d_tx_status), x,
                                         w.comp_status.as<uint8_t>());
          return e ? e : c.join_and_verify(s, x);
        });
  });
}

int cordahip_signed_txcomp_verify_device(cordahip_ctx* ctx, int device, const void* d_items, uint64_t n_items,
                                         uint32_t group, const void* d_payload, uint64_t payload_len,
                                         const void* d_tx_item_off, uint64_t ntx, const void* d_tx_sig_off,
                                         const void* d_scheme, const void* d_key, const void* d_key_off,
                                         uint64_t key_bytes, const void* d_sig, const void* d_sig_off,
                                         uint64_t sig_bytes, uint64_t nsig, void* d_txid, void* d_tx_status,
                                         void* d_first_bad, void* d_sig_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  sigpack::In in;
  if (!d || (ntx && (!d_tx_item_off || !d_tx_sig_off || !d_txid || !d_tx_status || !d_first_bad)) ||
      (n_items && !d_items) || (payload_len && !d_payload) ||
      !mixed_sigs(ctx, d_scheme, d_key, d_key_off, key_bytes, d_sig, d_sig_off, sig_bytes, nsig, d_sig_status, in))
    return CORDAHIP_ERR_INVALID_ARG;
  if (n_items >= (1ull << 31) - 1) return CORDAHIP_ERR_INVALID_ARG;  // the encoder's item slots and lists are 32-bit
  return guarded([&]() -> int {
    // as cordahip_signed_txcomp_verify_ed25519_device: a buffer set and the encoder's scratch
    SetLease lease(*d);
    TxSet& S = lease.get();
    std::lock_guard<std::mutex> gk(d->kryo_mu);
    TxWork& w = S.tx;
    const DeviceSignedTx c{*d,   S,      ntx,         d_tx_sig_off, nullptr,      nullptr,
                           nsig, d_txid, d_tx_status, d_first_bad,  d_sig_status, &in};
    return device_call(
        *d, hip_stream,
        [&] {
          const hipError_t e = c.prepare(n_items, true);
          return e ? e : kryo_scratch_ensure(*d, n_items, 0);
        },
        [&](hipStream_t s) {
          uint32_t* slots = d->kryo_items.as<uint32_t>();
          hipStream_t x = nullptr;
          hipError_t e = d->kryo_ev.wait(s);  // the previous users of the encoder's scratch are done
          e = e ? e : c.fork(s, x);
          e = e ? e : kryo_state_ready(*d, x);
          e = e ? e
                : launch_kryo_hash_chain(static_cast<const cordahip_kryo_item*>(d_items),
                                         static_cast<const uint8_t*>(d_payload), payload_len, n_items, group,
                                         d->kryo_fixed.as<uint8_t>(), slots, slots + n_items,
                                         d->kryo_sizes.as<uint64_t>(), w.comp_status.as<uint8_t>(),
                                         w.hashes.as<uint32_t>(), d->kryo_ws.as<uint8_t>(), kKryoDirectWriters, x);
          e = e ? e : kryo_usage_report(*d, nullptr, x);
          e = e ? e : d->kryo_ev.record(x);
          e = e ? e : launch_merkle_root(w.hashes.as<uint32_t>(), static_cast<const uint64_t*>(d_tx_item_off), ntx,
                                         static_cast<uint8_t*>(d_txid), static_cast<uint8_t*>(d_tx_status), x,
                                         w.comp_status.as<uint8_t>());
          return e ? e : c.join_and_verify(s, x);
        });
  });
}

}  // extern "C"
