// libcordahip.so's registered-key calls: the signer's and the verification keys'
// registries (cordahip_signer_*, cordahip_vkey_*), the host calls that sign and verify
// with them a chunk at a time (cordahip_sign, cordahip_ecdsa_sign, cordahip_verify_keyed,
// cordahip_ecdsa_verify_keyed, cordahip_rsa_verify_keyed) and their *_device forms. The shared runtime types are in
// runtime.hpp; the routed enqueues of the generic paths (K14, K15) in runtime.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "api_support.hpp"
#include "csr_check.hpp"
#include "ecdsa_sign_core.hpp"
#include "ecdsa_vkey.hpp"
#include "ed25519_comb.hpp"
#include "ed25519_vkey.hpp"
#include "pack_rows.hpp"
#include "rsa_vkey.hpp"

using namespace cordahip;
using namespace cordahip::rt;

namespace {

// What an add or a remove does on every device of the context, in order, each under its
// lock `mu` (Device::sign_mu or Device::vkey_mu) and counted as activity: build(d, i,
// more) on device i, which may clear `more` to end the round there; a later device
// whose answer does not agree with device 0's (agrees()) is CORDAHIP_ERR_HIP. The first
// failure ends the round and is returned, after undo(d) has run on every device visited,
// the failed one included, each current and under its lock.
template <class Build, class Agrees, class Undo>
int on_each_device(cordahip_ctx* ctx, std::mutex Device::*mu, Build build, Agrees agrees, Undo undo) {
  int rc = CORDAHIP_SUCCESS;
  size_t done = 0;
  bool more = true;
  for (; done < ctx->devs.size() && rc == CORDAHIP_SUCCESS && more; done++) {
    Device& d = *ctx->devs[done];
    std::lock_guard<std::mutex> gd(d.*mu);
    const Activity act(d);
    rc = build(d, done, more);
    if (rc == CORDAHIP_SUCCESS && done && !agrees()) rc = CORDAHIP_ERR_HIP;
  }
  if (rc == CORDAHIP_SUCCESS) return rc;
  for (size_t k = 0; k < done; k++) {
    Device& d = *ctx->devs[k];
    std::lock_guard<std::mutex> gd(d.*mu);
    if (hipSetDevice(d.id) == hipSuccess) undo(d);
  }
  return rc;
}
// a remove: clear(d) on every device, made current, whatever the devices before it
// answered; the first HIP error
template <class Clear>
int clear_on_each_device(cordahip_ctx* ctx, std::mutex Device::*mu, Clear clear) {
  hipError_t e = hipSuccess;
  (void)on_each_device(
      ctx, mu,
      [&](Device& d, size_t, bool&) {
        const hipError_t s = hipSetDevice(d.id);
        const hipError_t z = s ? s : clear(d);
        e = e ? e : z;
        return (int)CORDAHIP_SUCCESS;
      },
      [] { return true; }, [](Device&) {});
  return hip_err(e);
}

// ---- Ed25519 signing with registered keys (K11, ed25519_sign.hip) -------------
// A key's record zeroed on one device (sign_mu held, device current): after every
// signing kernel that may still read it; the stream is drained before return.
hipError_t signer_zero_record(Device& d, uint32_t slot) {
  if (!d.keys.tab.p && !d.ec_keys.tab.p) return hipSuccess;
  hipError_t e = hipSuccess;
  if (d.keys.tab.p) {
    e = d.keys.ev.sync();
    e = e ? e
          : hipMemsetAsync(d.keys.tab.as<uint32_t>() + (size_t)slot * kSignRecWords, 0, kSignRecWords * 4, d.stream);
  }
  if (d.ec_keys.tab.p) {  // the slot's record of the other family (K17): one pool, one remove
    EcSignKeys& k = d.ec_keys;
    hipError_t x = k.ev.sync();
    x = x ? x
          : hipMemsetAsync(k.tab.as<uint32_t>() + kEcSignRecBase + (size_t)slot * kEcSignRecWords, 0,
                           kEcSignRecWords * 4, d.stream);
    e = e ? e : x;
    if (k.scheme[slot]) k.live[k.scheme[slot] - 2]--;
    k.scheme[slot] = 0;
  }
  const hipError_t f = hipStreamSynchronize(d.stream);
  return e ? e : f;
}

// The seed expanded into the record of key_id's slot on one device (sign_mu held);
// pub: the device's A. The seed crosses in the device's page-locked stage, wiped
// here whatever happens; the kernel zeroes its device scratch.
int signer_expand_on(Device& d, const uint8_t seed[32], uint32_t key_id, uint8_t pub[32]) {
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  if (!d.keys.tab.p) {  // the first key of this device: the table, zeroed
    if (d.keys.tab.ensure(ed25519_keytab_bytes()) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
    if (hipMemsetAsync(d.keys.tab.p, 0, d.keys.tab.cap, d.stream) != hipSuccess) return CORDAHIP_ERR_HIP;
  }
  if (d.keys.stage.ensure(64) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
  uint8_t* stage = d.keys.stage.as<uint8_t>();
  uint32_t* tab = d.keys.tab.as<uint32_t>();
  std::memcpy(stage, seed, 32);
  hipError_t e = hipMemcpyAsync(tab + kSignSeedWord, stage, 32, hipMemcpyHostToDevice, d.stream);
  e = e ? e : launch_ed25519_key_expand(tab, key_id, d.comb(), d.stream);
  e = e ? e : hipMemcpyAsync(stage + 32, tab + kSignPubWord, 32, hipMemcpyDeviceToHost, d.stream);
  const hipError_t f = hipStreamSynchronize(d.stream);
  secure_wipe(stage, 32);
  if (e == hipSuccess && f == hipSuccess) std::memcpy(pub, stage + 32, 32);
  return hip_err(e ? e : f);
}

int signer_add_impl(cordahip_ctx* ctx, const uint8_t seed[32], uint32_t* key_id, uint8_t pub[32]) {
  auto& reg = ctx->signers;
  std::lock_guard<std::mutex> g(reg.mu);
  uint32_t slot, id;
  if (!reg.acquire(slot, id)) return CORDAHIP_ERR_OUT_OF_MEMORY;
  uint8_t first[32], cur[32];
  const int rc = on_each_device(
      ctx, &Device::sign_mu,
      [&](Device& d, size_t i, bool&) { return signer_expand_on(d, seed, id, i ? cur : first); },
      [&] { return std::memcmp(first, cur, 32) == 0; },
      [&](Device& d) {  // no device keeps a record of a key the caller never got
        if (!d.keys.tab.p) return;
        (void)signer_zero_record(d, slot);
        (void)hipMemsetAsync(d.keys.tab.as<uint32_t>() + kSignSeedWord, 0, 32, d.stream);
        (void)hipStreamSynchronize(d.stream);
      });
  if (rc != CORDAHIP_SUCCESS) return rc;
  reg.commit(slot);
  *key_id = id;
  std::memcpy(pub, first, 32);
  if (tracing()) fprintf(stderr, "[cordahip] signer: key id %u added (%u live)\n", id, reg.count);
  return CORDAHIP_SUCCESS;
}

int signer_remove_impl(cordahip_ctx* ctx, uint32_t key_id) {
  auto& reg = ctx->signers;
  std::lock_guard<std::mutex> g(reg.mu);
  uint32_t slot;
  if (!reg.release(key_id, slot)) return CORDAHIP_ERR_INVALID_ARG;
  // the id is dead from here on, whatever a device answers below
  const int rc = clear_on_each_device(ctx, &Device::sign_mu, [&](Device& d) { return signer_zero_record(d, slot); });
  if (tracing()) fprintf(stderr, "[cordahip] signer: key id %u removed (%u live)\n", key_id, reg.count);
  return rc;
}

// ---- ECDSA signing with registered keys (K17, ecdsa_sign_keyed.hip) -------------
// The key's record written in key_id's slot on one device (sign_mu held): the device's
// first ECDSA signer key allocates the table (records and scratch zeroed), its first
// key of a curve builds that curve's comb table. *taken: whether the device took d for
// a key (0 < d < n); pub: its Q = [d]G as X || Y. d crosses in the device's page-locked
// stage, wiped here whatever happens; the kernel zeroes its device scratch.
int ec_signer_add_on(Device& d, uint32_t scheme, const uint8_t key[32], uint32_t key_id, bool* taken,
                     uint8_t pub[64]) {
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  EcSignKeys& k = d.ec_keys;
  if (!k.tab.p) {
    if (k.tab.ensure(ecdsa_signtab_bytes()) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
    k.comb[0] = k.comb[1] = k.live[0] = k.live[1] = 0;
    std::memset(k.scheme, 0, sizeof k.scheme);
    if (hipMemsetAsync(k.tab.as<uint32_t>() + kEcSignRecBase, 0, (size_t)(kEcSignAllWords - kEcSignRecBase) * 4,
                       d.stream) != hipSuccess)
      return CORDAHIP_ERR_HIP;
  }
  uint32_t* tab = k.tab.as<uint32_t>();
  const bool build_comb = !k.comb[scheme - 2];  // marked built only once the stream has drained below
  if (build_comb && launch_ecdsa_sign_comb(tab, scheme, d.stream) != hipSuccess) return CORDAHIP_ERR_HIP;
  if (k.stage.ensure(128) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
  uint8_t* stage = k.stage.as<uint8_t>();
  std::memcpy(stage, key, 32);
  std::memset(stage + 32, 0, 96);
  hipError_t e = k.ev.sync();  // a removed key's slot: no kernel still reads its record
  e = e ? e : hipMemcpyAsync(tab + kEcSignKeyWord, stage, 32, hipMemcpyHostToDevice, d.stream);
  e = e ? e : launch_ecdsa_signer_add(tab, scheme, key_id, d.stream);
  e = e ? e : hipMemcpyAsync(stage + 32, tab + kEcSignOutWord, 80, hipMemcpyDeviceToHost, d.stream);
  const hipError_t f = hipStreamSynchronize(d.stream);
  secure_wipe(stage, 32);
  if (e == hipSuccess && f == hipSuccess) {
    uint32_t flag;
    std::memcpy(&flag, stage + 32, 4);
    *taken = flag == 1u;
    std::memcpy(pub, stage + 32 + 16, 64);
    if (build_comb) k.comb[scheme - 2] = 1;
    if (*taken) {
      const uint32_t slot = key_id & (kSignKeySlots - 1);
      k.scheme[slot] = (uint8_t)scheme;
      k.live[scheme - 2]++;
    }
  }
  return hip_err(e ? e : f);
}

int ec_signer_add_impl(cordahip_ctx* ctx, uint32_t scheme, const uint8_t key[32], uint32_t* key_id,
                       uint8_t* key_status, uint8_t pub[65]) {
  auto& reg = ctx->signers;
  std::lock_guard<std::mutex> g(reg.mu);
  uint32_t slot, id;
  if (!reg.acquire(slot, id)) return CORDAHIP_ERR_OUT_OF_MEMORY;
  bool first = false, cur = false;
  uint8_t pfirst[64], pcur[64];
  const int rc = on_each_device(
      ctx, &Device::sign_mu,
      [&](Device& d, size_t i, bool& more) {
        const int r = ec_signer_add_on(d, scheme, key, id, i ? &cur : &first, i ? pcur : pfirst);
        if (r == CORDAHIP_SUCCESS && !first) more = false;  // not a key: no device wrote a record
        return r;
      },
      [&] { return cur == first && std::memcmp(pfirst, pcur, 64) == 0; },
      [&](Device& d) {  // no device keeps a record of a key the caller never got
        if (!d.ec_keys.tab.p) return;
        (void)signer_zero_record(d, slot);
        (void)hipMemsetAsync(d.ec_keys.tab.as<uint32_t>() + kEcSignKeyWord, 0, 32, d.stream);
        (void)hipStreamSynchronize(d.stream);
      });
  if (rc != CORDAHIP_SUCCESS) return rc;
  if (!first) {
    *key_id = 0xFFFFFFFFu;
    *key_status = CORDAHIP_STATUS_BAD_KEY;
    return CORDAHIP_SUCCESS;
  }
  reg.commit(slot);
  *key_id = id;
  *key_status = CORDAHIP_STATUS_OK;
  pub[0] = 4;
  std::memcpy(pub + 1, pfirst, 64);
  if (tracing()) fprintf(stderr, "[cordahip] signer: ECDSA key id %u (scheme %u) added (%u live)\n", id, scheme, reg.count);
  return CORDAHIP_SUCCESS;
}

// One chunk of a registered-key host call: lanes [a, a + m) of the batch, their messages
// laid out as `lay` says (poff: the lanes' offsets in the stage when not dense), stream s.
struct KeyedChunk {
  uint64_t a, m;
  SignLayout lay;
  const uint64_t* poff;
  hipStream_t s;
};

// A registered-key host call for lanes [lo, hi) on one device, a chunk of
// CORDAHIP_HOST_CHUNK lanes (rounded up to `align`) at a time: the lanes packed into the
// stage's page-locked buffers (dense 32-byte rows when every message of the chunk is 32
// bytes -- the ids; else each message at a 16-byte-aligned offset with its length),
// across PCIe, the kernel, and the results back into the caller's arrays in lane order.
// The key ids, messages and statuses are the driver's; `call` (SignCall, VerifyCall)
// supplies the rest: ensure(c) sizes its stage buffers (true: out of memory), pack(c, x,
// y) packs rows [x, y), enqueue(c) issues its H2D copies and the kernel under the key
// table's lock, fetch(c) its D2H copy, deliver(c) copies its result out.
template <class Call>
int keyed_chunks(cordahip_ctx* ctx, Device& d, KeyedStage& st, const uint64_t* msg_off, uint8_t* status, uint64_t lo,
                 uint64_t hi, uint64_t align, const char* what, Call call) {
  std::lock_guard<std::mutex> g(st.mu);
  const NodeBind nb(d);
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  const uint64_t chunk = (env_lanes("CORDAHIP_HOST_CHUNK", 1ull << 22) + align - 1) / align * align;
  HostPool& pool = pool_of(ctx, d);
  std::vector<uint64_t> poff;
  for (uint64_t a = lo; a < hi; a += chunk) {
    const uint64_t m = std::min(chunk, hi - a);
    const double t0 = now_ms();
    poff.resize(m);
    const KeyedChunk c{a, m, msg_chunk_layout(msg_off, a, m, poff.data()), poff.data(), d.stream};
    const uint64_t bytes = c.lay.bytes;
    // the previous chunk has drained: growing frees nothing in use
    if (st.ids.ensure(m * 4) || st.msgs.ensure(std::max<uint64_t>(bytes, 16)) || st.msg_off.ensure(m * 8) ||
        st.msg_len.ensure(m * 4) || st.status.ensure(m) || call.ensure(c))
      return CORDAHIP_ERR_OUT_OF_MEMORY;
    pool.parallel_for(m, 1u << 14, [&](uint64_t x, uint64_t y) { call.pack(c, x, y); });
    hipError_t e = st.ids.to_device(m * 4, c.s);
    if (bytes) e = e ? e : st.msgs.to_device(bytes, c.s);
    if (!c.lay.dense) {
      e = e ? e : st.msg_off.to_device(m * 8, c.s);
      e = e ? e : st.msg_len.to_device(m * 4, c.s);
    }
    e = e ? e : call.enqueue(c);
    e = e ? e : call.fetch(c);
    e = e ? e : st.status.to_host(m, c.s);
    e = e ? e : st.ev.record(c.s);
    e = e ? e : st.ev.sync();
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(c.s);  // no queued work outlives the call
      return CORDAHIP_ERR_HIP;
    }
    call.deliver(c);
    std::memcpy(status + a, st.status.h.p, m);
    if (tracing())
      fprintf(stderr, "[cordahip] dev %d %s chunk: %llu lanes (%s messages) in %.2f ms\n", d.id, what,
              (unsigned long long)m, c.lay.dense ? "32-byte" : "CSR", now_ms() - t0);
  }
  return CORDAHIP_SUCCESS;
}

// The keyed signer on stream s (sign_mu held, device current): behind the table's
// previous user, followed by the table's fence. A device without a key table yet
// passes none: every ungated lane is then UNKNOWN_KEY.
hipError_t sign_enqueue(Device& d, const uint32_t* key_id, const uint8_t* msgs, const uint64_t* moff,
                        const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* gate, uint8_t* sigs,
                        uint8_t* status, hipStream_t s) {
  hipError_t e = d.keys.ev.wait(s);
  e = e ? e
        : launch_ed25519_sign_keyed(key_id, msgs, moff, mlen, msg_len, n, gate, d.keys.tab.as<uint32_t>(),
                                    d.comb(), sigs, status, s);
  return e ? e : d.keys.ev.record(s);
}

// cordahip_sign's part of a chunk (keyed_chunks): the gate bytes in, K11, the signature rows out.
struct SignCall {
  Device& d;
  const cordahip_sign_batch* b;
  KeyedStage& st;
  bool ensure(const KeyedChunk& c) { return st.gate.ensure(c.m) || st.sig_rows.ensure(c.m * 64); }
  void pack(const KeyedChunk& c, uint64_t x, uint64_t y) {
    sign_pack_rows(b, c.a, x, y, c.lay, c.poff, st.ids.h.as<uint32_t>(), st.gate.h.as<uint8_t>(),
                   st.msgs.h.as<uint8_t>(), st.msg_off.h.as<uint64_t>(), st.msg_len.h.as<uint32_t>());
  }
  hipError_t enqueue(const KeyedChunk& c) {
    if (b->gate)
      if (const hipError_t e = st.gate.to_device(c.m, c.s)) return e;
    const bool dense = c.lay.dense;
    std::lock_guard<std::mutex> gs(d.sign_mu);
    return sign_enqueue(d, st.ids.d.as<uint32_t>(), st.msgs.d.as<uint8_t>(),
                        dense ? nullptr : st.msg_off.d.as<uint64_t>(), dense ? nullptr : st.msg_len.d.as<uint32_t>(), 32,
                        c.m, b->gate ? st.gate.d.as<uint8_t>() : nullptr, st.sig_rows.d.as<uint8_t>(),
                        st.status.d.as<uint8_t>(), c.s);
  }
  hipError_t fetch(const KeyedChunk& c) { return st.sig_rows.to_host(c.m * 64, c.s); }
  void deliver(const KeyedChunk& c) { std::memcpy(b->sig + c.a * 64, st.sig_rows.h.p, c.m * 64); }
};

int sign_impl(cordahip_ctx* ctx, const cordahip_sign_batch* b) {
  const uint64_t n = b->n;
  if (n == 0) return CORDAHIP_SUCCESS;
  if (!b->key_id || !b->msg_off || !b->sig || !b->status) return CORDAHIP_ERR_INVALID_ARG;
  if (!check_sign_batch(PoolPar{*ctx->host}, b)) return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  if (b->msg_off[0] != b->msg_off[n] && !b->msg) return CORDAHIP_ERR_INVALID_ARG;
  return for_shards(ctx->devs, n, 64, [&](Device& d, uint64_t lo, uint64_t hi) {
    return keyed_chunks(ctx, d, d.sign_stage, b->msg_off, b->status, lo, hi, 1, "sign", SignCall{d, b, d.sign_stage});
  });
}

// The ECDSA keyed signer on stream s (sign_mu held, device current): behind the ECDSA
// table's previous user, followed by its fence. A device without that table passes
// none: every ungated lane is then UNKNOWN_KEY.
hipError_t ec_sign_enqueue(Device& d, const uint32_t* key_id, const uint8_t* msgs, const uint64_t* moff,
                           const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* gate, uint8_t* sigs,
                           uint8_t* sig_len, uint8_t* status, hipStream_t s) {
  const EcSignKeys& k = d.ec_keys;
  const bool have = k.tab.p != nullptr;
  hipError_t e = d.ec_keys.ev.wait(s);
  e = e ? e
        : launch_ecdsa_sign_keyed(key_id, msgs, moff, mlen, msg_len, n, gate, k.tab.as<uint32_t>(),
                                  have && k.live[0] > 0, have && k.live[1] > 0, sigs, sig_len, status, s);
  return e ? e : d.ec_keys.ev.record(s);
}

// cordahip_ecdsa_sign's part of a chunk (keyed_chunks): the gate bytes in, K17, the
// 72-byte DER slots and their lengths out.
struct EcSignCall {
  Device& d;
  const cordahip_ecdsa_sign_batch* b;
  KeyedStage& st;
  bool ensure(const KeyedChunk& c) {
    return st.gate.ensure(c.m) || st.sig_rows.ensure(c.m * kEcSignSigBytes) || st.sig_len.ensure(c.m);
  }
  void pack(const KeyedChunk& c, uint64_t x, uint64_t y) {
    sign_pack_rows(b, c.a, x, y, c.lay, c.poff, st.ids.h.as<uint32_t>(), st.gate.h.as<uint8_t>(),
                   st.msgs.h.as<uint8_t>(), st.msg_off.h.as<uint64_t>(), st.msg_len.h.as<uint32_t>());
  }
  hipError_t enqueue(const KeyedChunk& c) {
    if (b->gate)
      if (const hipError_t e = st.gate.to_device(c.m, c.s)) return e;
    const bool dense = c.lay.dense;
    std::lock_guard<std::mutex> gs(d.sign_mu);
    return ec_sign_enqueue(d, st.ids.d.as<uint32_t>(), st.msgs.d.as<uint8_t>(),
                           dense ? nullptr : st.msg_off.d.as<uint64_t>(), dense ? nullptr : st.msg_len.d.as<uint32_t>(),
                           32, c.m, b->gate ? st.gate.d.as<uint8_t>() : nullptr, st.sig_rows.d.as<uint8_t>(),
                           st.sig_len.d.as<uint8_t>(), st.status.d.as<uint8_t>(), c.s);
  }
  hipError_t fetch(const KeyedChunk& c) {
    const hipError_t e = st.sig_rows.to_host(c.m * kEcSignSigBytes, c.s);
    return e ? e : st.sig_len.to_host(c.m, c.s);
  }
  void deliver(const KeyedChunk& c) {
    std::memcpy(b->sig + c.a * kEcSignSigBytes, st.sig_rows.h.p, c.m * kEcSignSigBytes);
    std::memcpy(b->sig_len + c.a, st.sig_len.h.p, c.m);
  }
};

int ec_sign_impl(cordahip_ctx* ctx, const cordahip_ecdsa_sign_batch* b) {
  const uint64_t n = b->n;
  if (n == 0) return CORDAHIP_SUCCESS;
  if (!b->key_id || !b->msg_off || !b->sig || !b->sig_len || !b->status) return CORDAHIP_ERR_INVALID_ARG;
  if (!check_sign_batch(PoolPar{*ctx->host}, b)) return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  if (b->msg_off[0] != b->msg_off[n] && !b->msg) return CORDAHIP_ERR_INVALID_ARG;
  return for_shards(ctx->devs, n, 64, [&](Device& d, uint64_t lo, uint64_t hi) {
    return keyed_chunks(ctx, d, d.sign_stage, b->msg_off, b->status, lo, hi, 1, "ECDSA sign",
                        EcSignCall{d, b, d.sign_stage});
  });
}

// ---- Ed25519 verification against registered keys (K12, ed25519_vkey.hip) --------
// A key's record cleared on one device (vkey_mu held, device current): after every
// keyed kernel that may still read it; the stream is drained before return. The
// table's entries stay: without a record whose id matches, no lane reads them.
hipError_t vkey_clear_record(Device& d, uint32_t slot) {
  if (!d.vkeys.tab.p && !d.ec_vkeys.tab.p && !d.rsa_vkeys.tab.p) return hipSuccess;
  hipError_t e = hipSuccess;
  if (d.vkeys.tab.p) {
    d.vkeys.live &= ~(1ull << slot);  // routed enqueues (K14) count the device's live Ed25519 keys
    e = d.vkeys.ev.sync();
    e = e ? e
          : hipMemsetAsync(d.vkeys.tab.as<uint32_t>() + kVkeyRecBase + (size_t)slot * kVkeyRecWords, 0,
                           kVkeyRecWords * 4, d.stream);
  }
  if (d.ec_vkeys.tab.p) {  // the slot's record of the other family (K13): one pool, one remove
    hipError_t x = d.ec_vkeys.ev.sync();
    x = x ? x
          : hipMemsetAsync(d.ec_vkeys.tab.as<uint32_t>() + kEcVkeyRecBase + (size_t)slot * kEcVkeyRecWords, 0,
                           kEcVkeyRecWords * 4, d.stream);
    e = e ? e : x;
    EcVkeyState& st = d.ec_vkeys.state;
    if (st.scheme[slot]) st.live[st.scheme[slot] - 2]--;
    st.scheme[slot] = 0;
  }
  if (d.rsa_vkeys.tab.p) {  // and of the RSA family (K18)
    hipError_t x = d.rsa_vkeys.ev.sync();
    x = x ? x
          : hipMemsetAsync(d.rsa_vkeys.tab.as<uint8_t>() + (size_t)slot * sizeof(rsa::VkeyRecord), 0,
                           sizeof(rsa::VkeyRecord), d.stream);
    e = e ? e : x;
  }
  const hipError_t f = hipStreamSynchronize(d.stream);
  return e ? e : f;
}

// The key's record and table built in key_id's slot on one device (vkey_mu held);
// *decoded: whether the device took the bytes for a point.
int vkey_build_on(Device& d, const uint8_t key[32], uint32_t key_id, bool* decoded) {
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  if (!d.vkeys.tab.p) {  // the first key of this device: the tables; the records zeroed, the table of B built
    if (d.vkeys.tab.ensure(ed25519_vkey_bytes()) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
    if (hipMemsetAsync(d.vkeys.tab.as<uint32_t>() + kVkeyRecBase, 0, (kVkeyAllWords - kVkeyRecBase) * 4, d.stream) !=
            hipSuccess ||
        launch_ed25519_vkey_base(d.vkeys.tab.as<uint32_t>(), d.stream) != hipSuccess)
      return CORDAHIP_ERR_HIP;
  }
  if (d.vkeys.stage.ensure(64) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
  uint8_t* stage = d.vkeys.stage.as<uint8_t>();
  uint32_t* tab = d.vkeys.tab.as<uint32_t>();
  std::memcpy(stage, key, 32);
  std::memset(stage + 32, 0, 32);
  hipError_t e = d.vkeys.ev.sync();  // a removed key's slot: no kernel still reads its table
  e = e ? e : hipMemcpyAsync(tab + kVkeyKeyWord, stage, 32, hipMemcpyHostToDevice, d.stream);
  e = e ? e : launch_ed25519_vkey_build(tab, key_id, d.stream);
  e = e ? e : hipMemcpyAsync(stage + 32, tab + kVkeyOkWord, 32, hipMemcpyDeviceToHost, d.stream);
  const hipError_t f = hipStreamSynchronize(d.stream);
  if (e == hipSuccess && f == hipSuccess) {
    uint32_t flag;
    std::memcpy(&flag, stage + 32, 4);
    *decoded = flag == 1u;
    if (*decoded) d.vkeys.live |= 1ull << vkey_slot(key_id);
  }
  return hip_err(e ? e : f);
}

// The ECDSA key's record and table built in key_id's slot on one device (vkey_mu held):
// the device's first ECDSA key allocates the tables (records zeroed), its first key of a
// curve builds that curve's base-point table. *decoded: whether the device took the
// SEC1 bytes for a point of the curve (BC ECCurve.decodePoint).
int ec_vkey_build_on(Device& d, uint32_t scheme, const uint8_t* key, uint32_t key_len, uint32_t key_id, bool* decoded) {
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  EcVkeyState& st = d.ec_vkeys.state;
  if (!d.ec_vkeys.tab.p) {
    if (d.ec_vkeys.tab.ensure(ecdsa_vkey_bytes()) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
    st = EcVkeyState{};
    if (hipMemsetAsync(d.ec_vkeys.tab.as<uint32_t>() + kEcVkeyRecBase, 0, (kEcVkeyAllWords - kEcVkeyRecBase) * 4,
                       d.stream) != hipSuccess)
      return CORDAHIP_ERR_HIP;
  }
  uint32_t* tab = d.ec_vkeys.tab.as<uint32_t>();
  const bool build_base = !st.base[scheme - 2];  // marked built only once the stream has drained below
  if (build_base && launch_ecdsa_vkey_build(tab, scheme, ec_vkey_base_slot(scheme), 0u, 0u, d.stream) != hipSuccess)
    return CORDAHIP_ERR_HIP;
  if (d.ec_vkeys.stage.ensure(128) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
  uint8_t* stage = d.ec_vkeys.stage.as<uint8_t>();
  std::memset(stage, 0, 128);
  std::memcpy(stage, key, key_len);
  hipError_t e = d.ec_vkeys.ev.sync();  // a removed key's slot: no kernel still reads its table
  e = e ? e : hipMemcpyAsync(tab + kEcVkeyKeyWord, stage, 80, hipMemcpyHostToDevice, d.stream);
  e = e ? e : launch_ecdsa_vkey_build(tab, scheme, vkey_slot(key_id), key_id, key_len, d.stream);
  e = e ? e : hipMemcpyAsync(stage + 80, tab + kEcVkeyOkWord, 16, hipMemcpyDeviceToHost, d.stream);
  const hipError_t f = hipStreamSynchronize(d.stream);
  if (e == hipSuccess && f == hipSuccess) {
    uint32_t flag;
    std::memcpy(&flag, stage + 80, 4);
    *decoded = flag == 1u;
    if (build_base) st.base[scheme - 2] = 1;
    if (*decoded) {
      st.scheme[vkey_slot(key_id)] = (uint8_t)scheme;
      st.live[scheme - 2]++;
    }
  }
  return hip_err(e ? e : f);
}

// scheme 0: an Ed25519 key of 32 bytes (K12); 2 / 3: an ECDSA key in SEC1 form (K13).
// One pool of slots and one id space for both.
int vkey_add_impl(cordahip_ctx* ctx, uint32_t scheme, const uint8_t* key, uint32_t key_len, uint32_t* key_id,
                  uint8_t* key_status) {
  if (scheme && key_len != 33 && key_len != 65) {  // ECCurve.decodePoint: invalid point encoding
    *key_id = kVkeyNoId;
    *key_status = CORDAHIP_STATUS_BAD_KEY;
    return CORDAHIP_SUCCESS;
  }
  auto& reg = ctx->vkeys;
  std::lock_guard<std::mutex> g(reg.mu);
  uint32_t slot, id;
  if (!reg.acquire(slot, id)) return CORDAHIP_ERR_OUT_OF_MEMORY;
  bool first = false, cur = false;
  const int rc = on_each_device(
      ctx, &Device::vkey_mu,
      [&](Device& d, size_t i, bool& more) {
        const int r = scheme ? ec_vkey_build_on(d, scheme, key, key_len, id, i ? &cur : &first)
                             : vkey_build_on(d, key, id, i ? &cur : &first);
        if (r == CORDAHIP_SUCCESS && !first) more = false;  // not a point: no device wrote anything
        return r;
      },
      [&] { return cur == first; },
      [&](Device& d) { (void)vkey_clear_record(d, slot); });  // no device keeps a record of a key the caller never got
  if (rc != CORDAHIP_SUCCESS) return rc;
  if (!first) {
    *key_id = kVkeyNoId;
    *key_status = CORDAHIP_STATUS_BAD_KEY;
    return CORDAHIP_SUCCESS;
  }
  reg.commit(slot);
  *key_id = id;
  *key_status = CORDAHIP_STATUS_OK;
  if (tracing()) fprintf(stderr, "[cordahip] vkey: key id %u added (%u live)\n", id, reg.count);
  return CORDAHIP_SUCCESS;
}

// The RSA key's record, built by the host (rsa_vkey.hpp build_vkey_record), put in its
// id's slot on one device (vkey_mu held): the device's first RSA key allocates the table,
// zeroed. The record crosses in the table's page-locked stage, behind the table's fence.
int rsa_vkey_put_on(Device& d, const rsa::VkeyRecord& rec) {
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  RsaVerifyKeys& k = d.rsa_vkeys;
  if (!k.tab.p) {
    if (k.tab.ensure(rsa_vkey_bytes()) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
    if (hipMemsetAsync(k.tab.p, 0, k.tab.cap, d.stream) != hipSuccess) {
      k.tab.release();  // never a table that was not zeroed
      return CORDAHIP_ERR_HIP;
    }
  }
  if (k.stage.ensure(sizeof rec) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
  std::memcpy(k.stage.p, &rec, sizeof rec);
  hipError_t e = k.ev.sync();  // a removed key's slot: no kernel still reads its record
  e = e ? e
        : hipMemcpyAsync(k.tab.as<uint8_t>() + (size_t)vkey_slot(rec.id) * sizeof rec, k.stage.p, sizeof rec,
                         hipMemcpyHostToDevice, d.stream);
  const hipError_t f = hipStreamSynchronize(d.stream);
  return hip_err(e ? e : f);
}

// An RSA key (K18): the SPKI BIT STRING payload decoded as a generic lane's key is; the
// same pool of slots and the same id space as the other two families.
int rsa_vkey_add_impl(cordahip_ctx* ctx, const uint8_t* key, uint32_t key_len, uint32_t* key_id,
                      uint8_t* key_status) {
  rsa::VkeyRecord rec;
  const uint8_t ks = rsa::vkey_record_from_der(key, key_len, rec);
  if (ks != rsa::kOk) {  // BAD_KEY, or UNSUPPORTED for a key the GPU path declines: what a generic lane gets
    *key_id = kVkeyNoId;
    *key_status = ks;
    return CORDAHIP_SUCCESS;
  }
  auto& reg = ctx->vkeys;
  std::lock_guard<std::mutex> g(reg.mu);
  uint32_t slot, id;
  if (!reg.acquire(slot, id)) return CORDAHIP_ERR_OUT_OF_MEMORY;
  rec.id = id;
  const int rc = on_each_device(
      ctx, &Device::vkey_mu, [&](Device& d, size_t, bool&) { return rsa_vkey_put_on(d, rec); }, [] { return true; },
      [&](Device& d) { (void)vkey_clear_record(d, slot); });  // no device keeps a record of a key the caller never got
  if (rc != CORDAHIP_SUCCESS) return rc;
  {
    std::lock_guard<std::mutex> gm(ctx->rsa_mirror_mu);
    ctx->rsa_mirror[slot] = {id, rec.words, rec.bits};
  }
  reg.commit(slot);
  *key_id = id;
  *key_status = CORDAHIP_STATUS_OK;
  if (tracing())
    fprintf(stderr, "[cordahip] vkey: RSA key id %u (%u bits) added (%u live)\n", id, rec.bits, reg.count);
  return CORDAHIP_SUCCESS;
}

int vkey_remove_impl(cordahip_ctx* ctx, uint32_t key_id) {
  auto& reg = ctx->vkeys;
  std::lock_guard<std::mutex> g(reg.mu);
  uint32_t slot;
  if (!reg.release(key_id, slot)) return CORDAHIP_ERR_INVALID_ARG;
  {
    std::lock_guard<std::mutex> gm(ctx->rsa_mirror_mu);
    ctx->rsa_mirror[slot] = {};
  }
  // the id is dead from here on, whatever a device answers below
  const int rc = clear_on_each_device(ctx, &Device::vkey_mu, [&](Device& d) { return vkey_clear_record(d, slot); });
  if (tracing()) fprintf(stderr, "[cordahip] vkey: key id %u removed (%u live)\n", key_id, reg.count);
  return rc;
}

// The keyed verifier on stream s (vkey_mu held, device current): behind the tables'
// previous user, followed by the tables' fence. A device without key tables yet
// passes none: every lane is then UNKNOWN_KEY.
hipError_t vkey_enqueue(Device& d, const uint32_t* key_id, const uint8_t* sigs, const uint8_t* msgs,
                        const uint64_t* moff, const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* pre,
                        uint32_t flags, uint8_t* status, unsigned long long* verdict, hipStream_t s) {
  hipError_t e = d.vkeys.ev.wait(s);
  e = e ? e
        : launch_ed25519_verify_keyed(key_id, sigs, msgs, moff, mlen, msg_len, n, pre, flags,
                                      d.vkeys.tab.as<uint32_t>(), status, verdict, s);
  return e ? e : d.vkeys.ev.record(s);
}

// The ECDSA keyed verifier on stream s (vkey_mu held, device current): as vkey_enqueue,
// behind the ECDSA tables' fence. A device without ECDSA tables passes none: every lane
// is then UNKNOWN_KEY.
hipError_t ec_vkey_enqueue(Device& d, const uint32_t* key_id, const uint8_t* sigs, const uint8_t* sig_len,
                           const uint8_t* msgs, const uint64_t* moff, const uint32_t* mlen, uint32_t msg_len,
                           uint64_t n, const uint8_t* pre, uint32_t flags, uint8_t* status,
                           unsigned long long* verdict, hipStream_t s) {
  const EcVkeyState& st = d.ec_vkeys.state;
  const bool have = d.ec_vkeys.tab.p != nullptr;
  hipError_t e = d.ec_vkeys.ev.wait(s);
  e = e ? e
        : launch_ecdsa_verify_keyed(key_id, sigs, sig_len, msgs, moff, mlen, msg_len, n, pre, flags,
                                    d.ec_vkeys.tab.as<uint32_t>(), have && st.live[0] > 0, have && st.live[1] > 0,
                                    status, verdict, s);
  return e ? e : d.ec_vkeys.ev.record(s);
}

// The part of a chunk (keyed_chunks) of cordahip_verify_keyed (ec false: 64-byte
// signature rows, pack_rows.hpp keyed_pack_rows, K12) and of cordahip_ecdsa_verify_keyed
// (ec true: 72-byte DER slots with their lengths, keyed_ec_pack_rows, K13): the
// signature rows and the host's pre-statuses in, the kernel, the verdict words out.
// Shards start at multiples of 64 lanes and chunks are whole verdict words.
struct VerifyCall {
  Device& d;
  const cordahip_keyed_sig_batch* b;
  bool ec;
  KeyedStage& st;
  size_t row() const { return ec ? 72 : 64; }
  static uint64_t words(const KeyedChunk& c) { return (c.m + 63) / 64; }
  bool ensure(const KeyedChunk& c) {
    return st.sig_rows.ensure(c.m * row()) || st.pre.ensure(c.m) || st.verdict.ensure(words(c) * 8) ||
           (ec && st.sig_len.ensure(c.m));
  }
  void pack(const KeyedChunk& c, uint64_t x, uint64_t y) {
    uint8_t *hsig = st.sig_rows.h.as<uint8_t>(), *hpre = st.pre.h.as<uint8_t>(), *hm = st.msgs.h.as<uint8_t>();
    uint32_t *hid = st.ids.h.as<uint32_t>(), *hl = st.msg_len.h.as<uint32_t>();
    uint64_t* ho = st.msg_off.h.as<uint64_t>();
    if (ec) keyed_ec_pack_rows(b, c.a, x, y, c.lay, c.poff, hid, hsig, st.sig_len.h.as<uint8_t>(), hpre, hm, ho, hl);
    else keyed_pack_rows(b, c.a, x, y, c.lay, c.poff, hid, hsig, hpre, hm, ho, hl);
  }
  hipError_t enqueue(const KeyedChunk& c) {
    hipError_t e = st.sig_rows.to_device(c.m * row(), c.s);
    e = e ? e : st.pre.to_device(c.m, c.s);
    if (ec) e = e ? e : st.sig_len.to_device(c.m, c.s);
    if (e) return e;
    const uint8_t *sigs = st.sig_rows.d.as<uint8_t>(), *msgs = st.msgs.d.as<uint8_t>(), *pre = st.pre.d.as<uint8_t>();
    const uint32_t *ids = st.ids.d.as<uint32_t>(), *mlen = c.lay.dense ? nullptr : st.msg_len.d.as<uint32_t>();
    const uint64_t* moff = c.lay.dense ? nullptr : st.msg_off.d.as<uint64_t>();
    uint8_t* status = st.status.d.as<uint8_t>();
    unsigned long long* verdict = st.verdict.d.as<unsigned long long>();
    std::lock_guard<std::mutex> gs(d.vkey_mu);
    return ec ? ec_vkey_enqueue(d, ids, sigs, st.sig_len.d.as<uint8_t>(), msgs, moff, mlen, 32, c.m, pre, b->flags,
                                status, verdict, c.s)
              : vkey_enqueue(d, ids, sigs, msgs, moff, mlen, 32, c.m, pre, b->flags, status, verdict, c.s);
  }
  hipError_t fetch(const KeyedChunk& c) { return st.verdict.to_host(words(c) * 8, c.s); }
  void deliver(const KeyedChunk& c) {
    if (b->verdict) std::memcpy(b->verdict + c.a / 64, st.verdict.h.p, words(c) * 8);
  }
};

// what cordahip_verify_keyed and cordahip_ecdsa_verify_keyed ask of a batch (n > 0)
bool keyed_batch_ok(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* b) {
  const uint64_t n = b->n;
  if (!b->key_id || !b->sig_off || !b->msg_off || !b->status) return false;
  if (b->flags & ~CORDAHIP_FLAG_IS_VALID) return false;
  if (!check_keyed_sig_batch(PoolPar{*ctx->host}, b)) return false;  // before any enqueue
  return !((b->msg_off[0] != b->msg_off[n] && !b->msg) || (b->sig_off[0] != b->sig_off[n] && !b->sig));
}

int keyed_verify(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* b, bool ec) {
  if (b->n == 0) return CORDAHIP_SUCCESS;
  if (!keyed_batch_ok(ctx, b)) return CORDAHIP_ERR_INVALID_ARG;
  return for_shards(ctx->devs, b->n, 64, [&](Device& d, uint64_t lo, uint64_t hi) {
    return keyed_chunks(ctx, d, d.vkey_stage, b->msg_off, b->status, lo, hi, 64,
                        ec ? "keyed ECDSA verify" : "keyed verify", VerifyCall{d, b, ec, d.vkey_stage});
  });
}
int verify_keyed_impl(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* b) { return keyed_verify(ctx, b, false); }
int ec_verify_keyed_impl(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* b) { return keyed_verify(ctx, b, true); }

// The RSA keyed verifier on stream s (rsa_mu and vkey_mu held, device current, the RSA
// workspace grown for the call: rsa_ws_grow): behind the workspace's and the RSA table's
// previous users, followed by both fences. A device without an RSA table passes none:
// every lane is then UNKNOWN_KEY.
hipError_t rsa_vkey_enqueue(Device& d, const uint32_t* key_id, const uint8_t* sigs, const uint16_t* sig_len,
                            const uint8_t* msgs, const uint64_t* msg_off, uint32_t msg_len, uint32_t W, uint64_t n,
                            uint32_t flags, uint8_t* status, unsigned long long* verdict, hipStream_t s) {
  RsaWork& w = d.rsa;
  const size_t rb = rsa_ws_row_bytes(W);
  hipError_t e = w.ev.wait(s);
  e = e ? e : d.rsa_vkeys.ev.wait(s);
  e = e ? e
        : launch_rsa_verify_keyed(d.rsa_vkeys.tab.as<uint32_t>(), key_id, sigs, sig_len, msgs, msg_off, msg_len, W, n,
                                  status, verdict, w.ws.as<uint8_t>(), w.ws.cap / rb / 64 * 64, flags, s);
  const hipError_t r1 = w.ev.record(s), r2 = d.rsa_vkeys.ev.record(s);  // whatever was launched is fenced
  return e ? e : r1 ? r1 : r2;
}

// cordahip_rsa_verify_keyed for lanes [lo, hi) on one device, a chunk of
// CORDAHIP_HOST_CHUNK lanes at a time. A chunk's lanes are grouped by their key's width
// class from the context's mirror of the registry (a lane whose id is not live there is
// UNKNOWN_KEY now and is not sent); each class present runs over its rows only, in
// launches of at most kRsaKeyedRows rows through the keyed stage -- key ids, signatures
// right-sized to 4 W-byte slots, their lengths, the messages as a CSR of the launch's
// rows -- and the statuses go back to their lanes. The stage is single: a launch's
// statuses are read before the next one packs. rsa_mu is held for the run (the
// workspace), outside the stage's lock; vkey_mu per launch.
constexpr uint64_t kRsaKeyedRows = 1ull << 15;
int rsa_keyed_shard(cordahip_ctx* ctx, Device& d, const cordahip_keyed_sig_batch* b, uint64_t lo, uint64_t hi) {
  KeyedStage& st = d.vkey_stage;
  std::lock_guard<std::mutex> gr(d.rsa_mu);
  std::lock_guard<std::mutex> g(st.mu);
  const NodeBind nb(d);
  const Activity act(d);
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  const uint64_t chunk = (env_lanes("CORDAHIP_HOST_CHUNK", 1ull << 22) + 63) / 64 * 64;
  HostPool& pool = pool_of(ctx, d);
  hipStream_t s = d.stream;
  std::vector<uint64_t> cl[3], mo;  // lanes by class: 64, 96, 128 words
  cordahip_ctx::RsaVkeyMirror mir[kVkeySlots];
  for (uint64_t a = lo; a < hi; a += chunk) {
    const uint64_t m = std::min(chunk, hi - a);
    const double t0 = now_ms();
    {
      std::lock_guard<std::mutex> gm(ctx->rsa_mirror_mu);
      std::copy(ctx->rsa_mirror, ctx->rsa_mirror + kVkeySlots, mir);
    }
    for (auto& v : cl) v.clear();
    for (uint64_t i = a; i < a + m; i++) {
      const uint32_t id = b->key_id[i];
      const auto& k = mir[vkey_slot(id)];
      if (k.words && k.id == id) cl[k.words / 32 - 2].push_back(i);
      else b->status[i] = CORDAHIP_VERIFY_UNKNOWN_KEY;
    }
    for (int c = 0; c < 3; c++) {
      const uint32_t W = 64 + 32 * (uint32_t)c;
      for (uint64_t r0 = 0; r0 < cl[c].size(); r0 += kRsaKeyedRows) {
        const uint64_t rows = std::min<uint64_t>(kRsaKeyedRows, cl[c].size() - r0);
        const uint64_t* lanes = cl[c].data() + r0;
        mo.resize(rows + 1);
        mo[0] = 0;
        for (uint64_t r = 0; r < rows; r++) mo[r + 1] = mo[r] + (b->msg_off[lanes[r] + 1] - b->msg_off[lanes[r]]);
        // the previous launch has drained: growing frees nothing in use
        if (st.ids.ensure(rows * 4) || st.sig_rows.ensure(rows * 4 * W) || st.sig_len.ensure(rows * 2) ||
            st.msgs.ensure(std::max<uint64_t>(mo[rows], 16)) || st.msg_off.ensure((rows + 1) * 8) ||
            st.status.ensure(rows))
          return CORDAHIP_ERR_OUT_OF_MEMORY;
        std::memcpy(st.msg_off.h.p, mo.data(), (rows + 1) * 8);
        pool.parallel_for(rows, 256, [&](uint64_t x, uint64_t y) {
          for (uint64_t r = x; r < y; r++) {
            const uint64_t i = lanes[r];
            st.ids.h.as<uint32_t>()[r] = b->key_id[i];
            // a signature longer than the slot is longer than the modulus: its length
            // alone decides it (BAD_SIG), none of its bytes is sent
            const uint64_t sl = b->sig_off[i + 1] - b->sig_off[i], fit = sl <= 4ull * W ? sl : 0;
            uint8_t* row = st.sig_rows.h.as<uint8_t>() + r * 4ull * W;
            if (fit) std::memcpy(row, b->sig + b->sig_off[i], fit);
            std::memset(row + fit, 0, 4ull * W - fit);
            st.sig_len.h.as<uint16_t>()[r] = (uint16_t)std::min<uint64_t>(sl, 4ull * W + 1);
            if (mo[r + 1] != mo[r]) std::memcpy(st.msgs.h.as<uint8_t>() + mo[r], b->msg + b->msg_off[i], mo[r + 1] - mo[r]);
          }
        });
        hipError_t e = st.ids.to_device(rows * 4, s);
        e = e ? e : st.sig_rows.to_device(rows * 4 * W, s);
        e = e ? e : st.sig_len.to_device(rows * 2, s);
        if (mo[rows]) e = e ? e : st.msgs.to_device(mo[rows], s);
        e = e ? e : st.msg_off.to_device((rows + 1) * 8, s);
        if (e == hipSuccess && (e = rsa_ws_grow(d, W, rows)) == hipErrorOutOfMemory) {
          (void)hipStreamSynchronize(s);
          return CORDAHIP_ERR_OUT_OF_MEMORY;
        }
        if (e == hipSuccess) {
          std::lock_guard<std::mutex> gv(d.vkey_mu);
          e = rsa_vkey_enqueue(d, st.ids.d.as<uint32_t>(), st.sig_rows.d.as<uint8_t>(), st.sig_len.d.as<uint16_t>(),
                               st.msgs.d.as<uint8_t>(), st.msg_off.d.as<uint64_t>(), 0, W, rows, b->flags,
                               st.status.d.as<uint8_t>(), nullptr, s);
        }
        e = e ? e : st.status.to_host(rows, s);
        e = e ? e : st.ev.record(s);
        e = e ? e : st.ev.sync();
        if (e != hipSuccess) {
          (void)hipStreamSynchronize(s);  // no queued work outlives the call
          return CORDAHIP_ERR_HIP;
        }
        const uint8_t* hs = st.status.h.as<uint8_t>();
        for (uint64_t r = 0; r < rows; r++) b->status[lanes[r]] = hs[r];
      }
    }
    if (tracing())
      fprintf(stderr, "[cordahip] dev %d keyed RSA verify chunk: %llu lanes (%zu / %zu / %zu by class) in %.2f ms\n",
              d.id, (unsigned long long)m, cl[0].size(), cl[1].size(), cl[2].size(), now_ms() - t0);
  }
  // the shard's verdict words (shards start at multiples of 64 lanes)
  if (b->verdict) verdict_from_status(ctx, b->status + lo, hi - lo, b->verdict + lo / 64);
  return CORDAHIP_SUCCESS;
}

int rsa_verify_keyed_impl(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* b) {
  if (b->n == 0) return CORDAHIP_SUCCESS;
  if (!keyed_batch_ok(ctx, b)) return CORDAHIP_ERR_INVALID_ARG;
  return for_shards(ctx->devs, b->n, 64,
                    [&](Device& d, uint64_t lo, uint64_t hi) { return rsa_keyed_shard(ctx, d, b, lo, hi); });
}

// A device's cumulative counters of routed lanes: route_tot of the family's key table
// (K14: d.vkeys, K15: d.ec_vkeys), written by kernels the table's fence follows.
template <class Keys>
int route_stats(Device& d, const Keys& keys, uint64_t* keyed_lanes, uint64_t* generic_lanes) {
  std::lock_guard<std::mutex> g(d.vkey_mu);
  uint64_t tot[2] = {0, 0};
  if (keys.route_tot.p) {  // else: no routed enqueue of this family on this device yet
    // every routed enqueue's partition pass is followed by the table's fence
    if (hipSetDevice(d.id) != hipSuccess || keys.ev.sync() != hipSuccess ||
        hipMemcpy(tot, keys.route_tot.p, sizeof tot, hipMemcpyDeviceToHost) != hipSuccess)
      return CORDAHIP_ERR_HIP;
  }
  *keyed_lanes = tot[0];
  *generic_lanes = tot[1];
  return CORDAHIP_SUCCESS;
}

}  // namespace

extern "C" {

int cordahip_signer_add_ed25519(cordahip_ctx* ctx, const uint8_t seed[32], uint32_t* key_id, uint8_t pub[32]) {
  if (!ctx || !seed || !key_id || !pub) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return signer_add_impl(ctx, seed, key_id, pub); });
}

int cordahip_signer_remove(cordahip_ctx* ctx, uint32_t key_id) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return signer_remove_impl(ctx, key_id); });
}

int cordahip_sign(cordahip_ctx* ctx, const cordahip_sign_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return sign_impl(ctx, batch); });
}

int cordahip_sign_submit(cordahip_ctx* ctx, const cordahip_sign_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, sign_impl, batch);
}

int cordahip_ed25519_sign_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_msgs,
                                       uint32_t msg_len, uint64_t n, const void* d_gate, void* d_sigs,
                                       void* d_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (n && (!d_key_id || !d_sigs || !d_status || (msg_len && !d_msgs)))) return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_sigs) & 15) || (reinterpret_cast<uintptr_t>(d_key_id) & 3) ||
      (msg_len == 32 && (reinterpret_cast<uintptr_t>(d_msgs) & 15)))
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(d->sign_mu);
    return device_call(*d, hip_stream, [&](hipStream_t s) {
      return sign_enqueue(*d, static_cast<const uint32_t*>(d_key_id), static_cast<const uint8_t*>(d_msgs), nullptr,
                          nullptr, msg_len, n, static_cast<const uint8_t*>(d_gate), static_cast<uint8_t*>(d_sigs),
                          static_cast<uint8_t*>(d_status), s);
    });
  });
}

int cordahip_signer_add_ecdsa(cordahip_ctx* ctx, uint32_t scheme, const uint8_t d[32], uint32_t* key_id,
                              uint8_t* key_status, uint8_t pub[65]) {
  if (!ctx || !d || !key_id || !key_status || !pub) return CORDAHIP_ERR_INVALID_ARG;
  if (scheme != CORDAHIP_SCHEME_ECDSA_SECP256K1_SHA256 && scheme != CORDAHIP_SCHEME_ECDSA_SECP256R1_SHA256)
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return ec_signer_add_impl(ctx, scheme, d, key_id, key_status, pub); });
}

int cordahip_ecdsa_sign(cordahip_ctx* ctx, const cordahip_ecdsa_sign_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return ec_sign_impl(ctx, batch); });
}

int cordahip_ecdsa_sign_submit(cordahip_ctx* ctx, const cordahip_ecdsa_sign_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, ec_sign_impl, batch);
}

int cordahip_ecdsa_sign_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_msgs,
                                     uint32_t msg_len, uint64_t n, const void* d_gate, void* d_sigs,
                                     void* d_sig_len, void* d_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (n && (!d_key_id || !d_sigs || !d_sig_len || !d_status || (msg_len && !d_msgs))))
    return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_sigs) & 3) || (reinterpret_cast<uintptr_t>(d_key_id) & 3))
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(d->sign_mu);
    return device_call(*d, hip_stream, [&](hipStream_t s) {
      return ec_sign_enqueue(*d, static_cast<const uint32_t*>(d_key_id), static_cast<const uint8_t*>(d_msgs), nullptr,
                             nullptr, msg_len, n, static_cast<const uint8_t*>(d_gate), static_cast<uint8_t*>(d_sigs),
                             static_cast<uint8_t*>(d_sig_len), static_cast<uint8_t*>(d_status), s);
    });
  });
}

int cordahip_vkey_add_ed25519(cordahip_ctx* ctx, const uint8_t key[32], uint32_t* key_id, uint8_t* key_status) {
  if (!ctx || !key || !key_id || !key_status) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return vkey_add_impl(ctx, 0u, key, 32u, key_id, key_status); });
}

int cordahip_vkey_add_ecdsa(cordahip_ctx* ctx, uint32_t scheme, const uint8_t* key, uint32_t key_len, uint32_t* key_id,
                            uint8_t* key_status) {
  if (!ctx || !key_id || !key_status || (key_len && !key)) return CORDAHIP_ERR_INVALID_ARG;
  if (scheme != CORDAHIP_SCHEME_ECDSA_SECP256K1_SHA256 && scheme != CORDAHIP_SCHEME_ECDSA_SECP256R1_SHA256)
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return vkey_add_impl(ctx, scheme, key, key_len, key_id, key_status); });
}

int cordahip_vkey_remove(cordahip_ctx* ctx, uint32_t key_id) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return vkey_remove_impl(ctx, key_id); });
}

int cordahip_vkey_set_routing(cordahip_ctx* ctx, uint32_t on) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  for (auto& dp : ctx->devs) dp->route_on.store(on ? 1u : 0u);
  return CORDAHIP_SUCCESS;
}

int cordahip_vkey_route_stats(cordahip_ctx* ctx, int device, uint64_t* keyed_lanes, uint64_t* generic_lanes) {
  Device* d = dev_at(ctx, device);
  if (!d || !keyed_lanes || !generic_lanes) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return route_stats(*d, d->vkeys, keyed_lanes, generic_lanes); });
}

int cordahip_vkey_set_routing_ecdsa(cordahip_ctx* ctx, uint32_t on) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  for (auto& dp : ctx->devs) dp->ec_route_on.store(on ? 1u : 0u);
  return CORDAHIP_SUCCESS;
}

int cordahip_vkey_route_stats_ecdsa(cordahip_ctx* ctx, int device, uint64_t* keyed_lanes, uint64_t* generic_lanes) {
  Device* d = dev_at(ctx, device);
  if (!d || !keyed_lanes || !generic_lanes) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return route_stats(*d, d->ec_vkeys, keyed_lanes, generic_lanes); });
}

int cordahip_verify_keyed(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return verify_keyed_impl(ctx, batch); });
}

int cordahip_verify_keyed_submit(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, verify_keyed_impl, batch);
}

int cordahip_ed25519_verify_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_sigs,
                                         const void* d_msgs, uint32_t msg_len, uint64_t n, void* d_status,
                                         void* d_verdict, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (n && (!d_key_id || !d_sigs || !d_status || (msg_len && !d_msgs)))) return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_sigs) & 15) || (reinterpret_cast<uintptr_t>(d_key_id) & 3) ||
      (reinterpret_cast<uintptr_t>(d_verdict) & 7) || (msg_len == 32 && (reinterpret_cast<uintptr_t>(d_msgs) & 15)))
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(d->vkey_mu);
    return device_call(*d, hip_stream, [&](hipStream_t s) {
      return vkey_enqueue(*d, static_cast<const uint32_t*>(d_key_id), static_cast<const uint8_t*>(d_sigs),
                          static_cast<const uint8_t*>(d_msgs), nullptr, nullptr, msg_len, n, nullptr, 0u,
                          static_cast<uint8_t*>(d_status), static_cast<unsigned long long*>(d_verdict), s);
    });
  });
}

int cordahip_ecdsa_verify_keyed(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return ec_verify_keyed_impl(ctx, batch); });
}

int cordahip_ecdsa_verify_keyed_submit(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, ec_verify_keyed_impl, batch);
}

int cordahip_ecdsa_verify_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_sigs,
                                       const void* d_sig_len, const void* d_msgs, uint32_t msg_len, uint64_t n,
                                       void* d_status, void* d_verdict, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (n && (!d_key_id || !d_sigs || !d_sig_len || !d_status || (msg_len && !d_msgs))))
    return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_key_id) & 3) || (reinterpret_cast<uintptr_t>(d_verdict) & 7))
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(d->vkey_mu);
    return device_call(*d, hip_stream, [&](hipStream_t s) {
      return ec_vkey_enqueue(*d, static_cast<const uint32_t*>(d_key_id), static_cast<const uint8_t*>(d_sigs),
                             static_cast<const uint8_t*>(d_sig_len), static_cast<const uint8_t*>(d_msgs), nullptr,
                             nullptr, msg_len, n, nullptr, 0u, static_cast<uint8_t*>(d_status),
                             static_cast<unsigned long long*>(d_verdict), s);
    });
  });
}

int cordahip_vkey_add_rsa(cordahip_ctx* ctx, const uint8_t* key, uint32_t key_len, uint32_t* key_id,
                          uint8_t* key_status) {
  if (!ctx || !key || !key_id || !key_status) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return rsa_vkey_add_impl(ctx, key, key_len, key_id, key_status); });
}

int cordahip_rsa_verify_keyed(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return rsa_verify_keyed_impl(ctx, batch); });
}

int cordahip_rsa_verify_keyed_submit(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, rsa_verify_keyed_impl, batch);
}

int cordahip_rsa_verify_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_sigs,
                                     const void* d_sig_len, const void* d_msgs, uint32_t msg_len, uint32_t mod_words,
                                     uint64_t n, void* d_status, void* d_verdict, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (mod_words != 64 && mod_words != 96 && mod_words != 128) ||
      (n && (!d_key_id || !d_sigs || !d_sig_len || !d_status || (msg_len && !d_msgs))))
    return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_key_id) & 3) || (reinterpret_cast<uintptr_t>(d_sig_len) & 1) ||
      (reinterpret_cast<uintptr_t>(d_verdict) & 7))
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(d->rsa_mu);
    return device_call(
        *d, hip_stream, [&] { return rsa_ws_grow(*d, mod_words, n); },
        [&](hipStream_t s) {
          std::lock_guard<std::mutex> gv(d->vkey_mu);
          return rsa_vkey_enqueue(*d, static_cast<const uint32_t*>(d_key_id), static_cast<const uint8_t*>(d_sigs),
                                  static_cast<const uint16_t*>(d_sig_len), static_cast<const uint8_t*>(d_msgs),
                                  nullptr, msg_len, mod_words, n, 0u, static_cast<uint8_t*>(d_status),
                                  static_cast<unsigned long long*>(d_verdict), s);
        });
  });
}

int cordahip_rsa_public_op_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_in,
                                        uint32_t mod_words, uint64_t n, void* d_out, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (mod_words != 64 && mod_words != 96 && mod_words != 128) || (n && (!d_key_id || !d_in || !d_out)))
    return CORDAHIP_ERR_INVALID_ARG;
  if ((reinterpret_cast<uintptr_t>(d_key_id) | reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 3)
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(d->vkey_mu);  // no workspace: the table's lock and fence alone
    return device_call(*d, hip_stream, [&](hipStream_t s) {
      hipError_t e = d->rsa_vkeys.ev.wait(s);
      e = e ? e
            : launch_rsa_public_op_keyed(d->rsa_vkeys.tab.as<uint32_t>(), static_cast<const uint32_t*>(d_key_id),
                                         static_cast<const uint32_t*>(d_in), mod_words, n,
                                         static_cast<uint32_t*>(d_out), s);
      const hipError_t r = d->rsa_vkeys.ev.record(s);
      return e ? e : r;
    });
  });
}

}  // extern "C"
