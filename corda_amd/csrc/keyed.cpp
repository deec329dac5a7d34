// libcordahip.so's registered-key calls: the signer's and the verification keys'
// registries (cordahip_signer_*, cordahip_vkey_*), the host calls that sign and verify
// with them a chunk at a time (cordahip_sign, cordahip_ecdsa_sign, cordahip_verify_keyed,
// cordahip_ecdsa_verify_keyed, cordahip_rsa_verify_keyed, cordahip_rsa_sign) and their *_device forms. The shared runtime types are in
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
#include "rsa_sign.hpp"
#include "rsa_vkey.hpp"

using namespace cordahip;
using namespace cordahip::rt;

// What each family's table holds for a slot, and of the signer's what is secret
// (runtime.hpp KeyTable), from the kernels' layouts.
namespace cordahip {
namespace rt {
TabSpan SignKeys::record(uint32_t slot) const { return {(size_t)slot * kSignRecWords * 4, kSignRecWords * 4}; }
TabSpan SignKeys::secrets() const { return {0, tab.cap}; }
TabSpan EcSignKeys::record(uint32_t slot) const {
  return {(kEcSignRecBase + (size_t)slot * kEcSignRecWords) * 4, kEcSignRecWords * 4};
}
TabSpan EcSignKeys::secrets() const {  // the records and the scratch; the comb tables before them are public
  return {(size_t)kEcSignRecBase * 4, (size_t)(kEcSignAllWords - kEcSignRecBase) * 4};
}
TabSpan RsaSignKeys::record(uint32_t slot) const {  // no RSA key in the slot: its index word, a hint no lane trusts
  if (!rec_of[slot]) return {(size_t)(rsa::kSignTabIdxWord + slot) * 4, 4};
  return {(rsa::kSignTabRecBase + (size_t)(rec_of[slot] - 1) * rsa::kSignRecWords) * 4, sizeof(rsa::SignRecord)};
}
TabSpan RsaSignKeys::secrets() const {  // the records and the scratch; the index before them is public
  return {(size_t)rsa::kSignTabRecBase * 4, rsa::kSignTabBytes - (size_t)rsa::kSignTabRecBase * 4};
}
TabSpan VerifyKeys::record(uint32_t slot) const {
  return {(kVkeyRecBase + (size_t)slot * kVkeyRecWords) * 4, kVkeyRecWords * 4};
}
TabSpan EcVerifyKeys::record(uint32_t slot) const {
  return {(kEcVkeyRecBase + (size_t)slot * kEcVkeyRecWords) * 4, kEcVkeyRecWords * 4};
}
TabSpan RsaVerifyKeys::record(uint32_t slot) const {
  return {(size_t)slot * sizeof(rsa::VkeyRecord), sizeof(rsa::VkeyRecord)};
}
}  // namespace rt
}  // namespace cordahip

namespace {

// What an add does on every device of the context, in order, each under its
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
// A slot's record cleared on one device in every allocated family of a registry -- the
// signer's (sign_mu held) or the verification keys' (vkey_mu held), device current: one
// pool of slots, one remove. Each family's fence is waited for before its record is
// zeroed, so no kernel still reads it, and the host's note of the slot goes with it
// (KeyTable); every family is visited whatever an earlier one answered, and the stream
// is drained before return. The first error.
enum class Registry { kSigner, kVerify };
hipError_t clear_slot(Device& d, Registry which, uint32_t slot) {
  hipError_t e = hipSuccess;
  bool any = false;
  const auto clear = [&](auto& k) {
    if (!k.tab.p) return;
    any = true;
    const TabSpan r = k.record(slot);  // before the note goes: the RSA signer's says where the record is
    k.forget(slot);
    hipError_t x = k.ev.sync();
    x = x ? x : hipMemsetAsync(k.tab.template as<uint8_t>() + r.at, 0, r.bytes, d.stream);
    e = e ? e : x;
  };
  if (which == Registry::kSigner) d.signer_keys(clear);
  else d.verify_keys(clear);
  if (!any) return hipSuccess;
  const hipError_t f = hipStreamSynchronize(d.stream);
  return e ? e : f;
}
// a remove: the slot cleared on every device, each made current under the registry's
// lock, whatever the devices before it answered; the first HIP error
int clear_slot_on_each_device(cordahip_ctx* ctx, Registry which, uint32_t slot) {
  hipError_t e = hipSuccess;
  for (auto& dp : ctx->devs) {
    Device& d = *dp;
    std::lock_guard<std::mutex> gd(which == Registry::kSigner ? d.sign_mu : d.vkey_mu);
    const Activity act(d);
    const hipError_t s = hipSetDevice(d.id);
    const hipError_t z = s ? s : clear_slot(d, which, slot);
    e = e ? e : z;
  }
  return hip_err(e);
}

// ---- Ed25519 signing with registered keys (K11, ed25519_sign.hip) -------------

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
        (void)clear_slot(d, Registry::kSigner, slot);
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
  {
    std::lock_guard<std::mutex> gm(ctx->rsa_mirror_mu);
    if (ctx->rsa_sign_mirror[slot].words) ctx->rsa_signers--;
    ctx->rsa_sign_mirror[slot] = {};
  }
  // the id is dead from here on, whatever a device answers below
  const int rc = clear_slot_on_each_device(ctx, Registry::kSigner, slot);
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
    k.book = {};
    if (hipMemsetAsync(k.tab.as<uint32_t>() + kEcSignRecBase, 0, (size_t)(kEcSignAllWords - kEcSignRecBase) * 4,
                       d.stream) != hipSuccess)
      return CORDAHIP_ERR_HIP;
  }
  uint32_t* tab = k.tab.as<uint32_t>();
  const bool build_comb = !k.book.table_built(scheme);  // marked built only once the stream has drained below
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
    if (build_comb) k.book.mark_built(scheme);
    if (*taken) k.book.take(key_id & (kSignKeySlots - 1), scheme);
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
        (void)clear_slot(d, Registry::kSigner, slot);
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


// ---- RSA signing with registered private keys (K19, rsa_sign_keyed.hip) ----------
// The key's record, built by the host (rsa_sign.hpp build_sign_record), put into a free
// record of the table on one device (sign_mu held) with the slot's index word, and
// tried: the kernel signs the fixed EM of rsa_sign.hpp consistency_em in the table's
// scratch and checks it with the public key, which is what catches a dP, dQ or qInv
// that does not belong to p, q and e. *consistent: whether it did; if not, the record
// and the slot's index word are zeroed again here. A table that this add allocated is
// released whenever the add does not end in an accepted key on this device -- turned
// down, out of memory for the stage, or a HIP error: such an add leaves no memory behind. The device's first RSA signing key allocates the
// table, zeroed.
// The record crosses in the table's page-locked stage, wiped here whatever happens.
int rsa_signer_put_on(Device& d, const rsa::SignRecord& rec, uint32_t slot, bool* consistent) {
  if (hipSetDevice(d.id) != hipSuccess) return CORDAHIP_ERR_HIP;
  RsaSignKeys& k = d.rsa_keys;
  const bool fresh = !k.tab.p;
  if (fresh) {
    if (k.tab.ensure(rsa_signtab_bytes()) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
    std::memset(k.rec_of, 0, sizeof k.rec_of);
    std::memset(k.used, 0, sizeof k.used);
    if (hipMemsetAsync(k.tab.p, 0, k.tab.cap, d.stream) != hipSuccess) {
      k.tab.release();  // never a table that was not zeroed
      return CORDAHIP_ERR_HIP;
    }
  }
  // a table this add allocated goes again with an add that fails or is turned down: the
  // stream drained first, so no copy or kernel still has it (sign_mu is held)
  const auto drop_fresh = [&] {
    if (!fresh) return;
    k.forget(slot);
    (void)hipStreamSynchronize(d.stream);
    k.tab.release();
  };
  constexpr size_t kScr = (size_t)(rsa::kSignTabWords - rsa::kSignTabScratch) * 4;
  if (k.stage.ensure(sizeof rec + kScr + 16) != hipSuccess) {
    drop_fresh();
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  }
  const int r = k.take(slot);
  if (r < 0) {
    drop_fresh();
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  }
  uint8_t* st = k.stage.as<uint8_t>();
  uint32_t* scr = reinterpret_cast<uint32_t*>(st + sizeof rec);
  uint32_t* tail = scr + kScr / 4;  // the index word out, the answer back
  std::memcpy(st, &rec, sizeof rec);
  std::memset(scr, 0, kScr + 16);
  scr[rsa::kSignScrIdWord - rsa::kSignTabScratch] = rec.id;
  rsa::consistency_em(rec.bits, rec.words, scr + (rsa::kSignScrEmWord - rsa::kSignTabScratch));
  tail[0] = (uint32_t)r + 1;
  tail[1] = 0xffu;
  uint32_t* tab = k.tab.as<uint32_t>();
  uint32_t* drec = tab + rsa::kSignTabRecBase + (size_t)r * rsa::kSignRecWords;
  hipError_t e = k.ev.sync();  // a removed key's record: no kernel still reads it
  e = e ? e : hipMemcpyAsync(drec, st, sizeof rec, hipMemcpyHostToDevice, d.stream);
  e = e ? e : hipMemcpyAsync(tab + rsa::kSignTabIdxWord + slot, tail, 4, hipMemcpyHostToDevice, d.stream);
  e = e ? e : hipMemcpyAsync(tab + rsa::kSignTabScratch, scr, kScr, hipMemcpyHostToDevice, d.stream);
  e = e ? e : launch_rsa_sign_selftest(tab, rec.words, d.stream);
  e = e ? e : hipMemcpyAsync(tail + 1, tab + rsa::kSignScrStatusWord, 4, hipMemcpyDeviceToHost, d.stream);
  hipError_t f = hipStreamSynchronize(d.stream);
  secure_wipe(st, sizeof rec);
  if (e == hipSuccess && f == hipSuccess) {
    *consistent = (tail[1] & 0xffu) == CORDAHIP_STATUS_OK;
    if (!*consistent) {  // the record and the slot's index word zeroed again
      k.forget(slot);
      e = hipMemsetAsync(drec, 0, sizeof rec, d.stream);
      e = e ? e : hipMemsetAsync(tab + rsa::kSignTabIdxWord + slot, 0, 4, d.stream);
      f = hipStreamSynchronize(d.stream);
      drop_fresh();
    }
  } else {
    drop_fresh();  // else the caller's undo clears the slot in the table that stays
  }
  return hip_err(e ? e : f);
}

int rsa_signer_add_impl(cordahip_ctx* ctx, const cordahip_rsa_private_key* key, uint32_t* key_id,
                        uint8_t* key_status, uint8_t modulus[512], uint32_t* modulus_len) {
  rsa::SignRecord rec;
  struct Wipe {  // the host's copy of the components goes whatever the add answers
    rsa::SignRecord& r;
    ~Wipe() { secure_wipe(&r, sizeof r); }
  } wipe{rec};
  const rsa::PrivateKeyIn in{key->p,     key->q,      key->dp,     key->dq,       key->qinv, key->p_len,
                             key->q_len, key->dp_len, key->dq_len, key->qinv_len, key->e};
  uint8_t ks = rsa::build_sign_record(in, rec);
  const auto declined = [&] {  // BAD_KEY, or UNSUPPORTED for a key the GPU path declines: data, no slot taken
    *key_id = 0xFFFFFFFFu;
    *key_status = ks;
    return CORDAHIP_SUCCESS;
  };
  if (ks != rsa::kOk) return declined();
  auto& reg = ctx->signers;
  std::lock_guard<std::mutex> g(reg.mu);
  if (ctx->rsa_signers >= CORDAHIP_RSA_SIGNER_MAX_KEYS) return CORDAHIP_ERR_OUT_OF_MEMORY;
  uint32_t slot, id;
  if (!reg.acquire(slot, id)) return CORDAHIP_ERR_OUT_OF_MEMORY;
  rec.id = id;
  bool first = false, cur = false;
  const int rc = on_each_device(
      ctx, &Device::sign_mu,
      [&](Device& d, size_t i, bool& more) {
        const int r = rsa_signer_put_on(d, rec, slot, i ? &cur : &first);
        if (r == CORDAHIP_SUCCESS && !first) more = false;  // inconsistent: no device keeps the record
        return r;
      },
      [&] { return cur == first; },
      [&](Device& d) {  // no device keeps a record of a key the caller never got
        if (d.rsa_keys.tab.p) (void)clear_slot(d, Registry::kSigner, slot);
      });
  if (rc != CORDAHIP_SUCCESS) return rc;
  if (!first) {
    ks = CORDAHIP_STATUS_BAD_KEY;
    return declined();
  }
  {
    std::lock_guard<std::mutex> gm(ctx->rsa_mirror_mu);
    ctx->rsa_sign_mirror[slot] = {id, rec.words, rec.bits};
  }
  ctx->rsa_signers++;
  reg.commit(slot);
  *key_id = id;
  *key_status = CORDAHIP_STATUS_OK;
  const uint32_t k = (rec.bits + 7) / 8;
  std::memset(modulus, 0, 512);
  for (uint32_t b = 0; b < k; b++) modulus[k - 1 - b] = (uint8_t)(rec.n[b >> 2] >> (8 * (b & 3)));
  *modulus_len = k;
  if (tracing())
    fprintf(stderr, "[cordahip] signer: RSA key id %u (%u bits) added (%u live)\n", id, rec.bits, reg.count);
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

// The prologue of a registered-key host call's shard on one device: the stage's lock,
// held for the shard's run; the thread bound to the device's NUMA node; the run counted
// as activity; the device current (ok: it is); the chunk size, CORDAHIP_HOST_CHUNK lanes
// rounded up to `align`; the device's host pool.
struct ShardRun {
  std::lock_guard<std::mutex> g;
  const NodeBind nb;
  const Activity act;
  const bool ok;
  const uint64_t chunk;
  HostPool& pool;
  ShardRun(cordahip_ctx* ctx, Device& d, KeyedStage& st, uint64_t align)
      : g(st.mu), nb(d), act(d), ok(hipSetDevice(d.id) == hipSuccess),
        chunk((env_lanes("CORDAHIP_HOST_CHUNK", 1ull << 22) + align - 1) / align * align), pool(pool_of(ctx, d)) {}
};

// One round trip of packed rows through the stage on stream s: work() issues the copies
// in, the kernel (under the key table's lock) and the call's own copies out; the `rows`
// statuses follow, st.ev is recorded after that last copy and the host waits for it. On
// any HIP error the stream is drained first -- no queued work outlives the call -- and
// the answer is CORDAHIP_ERR_HIP.
template <class Work>
int round_trip(KeyedStage& st, uint64_t rows, hipStream_t s, Work work) {
  hipError_t e = work();
  e = e ? e : st.status.to_host(rows, s);
  e = e ? e : st.ev.record(s);
  e = e ? e : st.ev.sync();
  if (e == hipSuccess) return CORDAHIP_SUCCESS;
  (void)hipStreamSynchronize(s);
  return CORDAHIP_ERR_HIP;
}

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
  ShardRun run(ctx, d, st, align);
  if (!run.ok) return CORDAHIP_ERR_HIP;
  std::vector<uint64_t> poff;
  for (uint64_t a = lo; a < hi; a += run.chunk) {
    const uint64_t m = std::min(run.chunk, hi - a);
    const double t0 = now_ms();
    poff.resize(m);
    const KeyedChunk c{a, m, msg_chunk_layout(msg_off, a, m, poff.data()), poff.data(), d.stream};
    const uint64_t bytes = c.lay.bytes;
    // the previous chunk has drained: growing frees nothing in use
    if (st.ids.ensure(m * 4) || st.msgs.ensure(std::max<uint64_t>(bytes, 16)) || st.msg_off.ensure(m * 8) ||
        st.msg_len.ensure(m * 4) || st.status.ensure(m) || call.ensure(c))
      return CORDAHIP_ERR_OUT_OF_MEMORY;
    run.pool.parallel_for(m, 1u << 14, [&](uint64_t x, uint64_t y) { call.pack(c, x, y); });
    const int rc = round_trip(st, m, c.s, [&] {
      hipError_t e = st.ids.to_device(m * 4, c.s);
      if (bytes) e = e ? e : st.msgs.to_device(bytes, c.s);
      if (!c.lay.dense) {
        e = e ? e : st.msg_off.to_device(m * 8, c.s);
        e = e ? e : st.msg_len.to_device(m * 4, c.s);
      }
      e = e ? e : call.enqueue(c);
      return e ? e : call.fetch(c);
    });
    if (rc != CORDAHIP_SUCCESS) return rc;
    call.deliver(c);
    std::memcpy(status + a, st.status.h.p, m);
    if (tracing())
      fprintf(stderr, "[cordahip] dev %d %s chunk: %llu lanes (%s messages) in %.2f ms\n", d.id, what,
              (unsigned long long)m, c.lay.dense ? "32-byte" : "CSR", now_ms() - t0);
  }
  return CORDAHIP_SUCCESS;
}

// The keyed signers on stream s (sign_mu held, device current), each behind its table's
// previous user and followed by the table's fence (fenced): Ed25519 (K11) and ECDSA
// (K17). A device without the family's table yet passes none: every ungated lane is
// then UNKNOWN_KEY.
hipError_t sign_enqueue(Device& d, const uint32_t* key_id, const uint8_t* msgs, const uint64_t* moff,
                        const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* gate, uint8_t* sigs,
                        uint8_t* status, hipStream_t s) {
  return fenced({&d.keys.ev}, s, [&] {
    return launch_ed25519_sign_keyed(key_id, msgs, moff, mlen, msg_len, n, gate, d.keys.tab.as<uint32_t>(), d.comb(),
                                     sigs, status, s);
  });
}
hipError_t ec_sign_enqueue(Device& d, const uint32_t* key_id, const uint8_t* msgs, const uint64_t* moff,
                           const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* gate, uint8_t* sigs,
                           uint8_t* sig_len, uint8_t* status, hipStream_t s) {
  const EcSignKeys& k = d.ec_keys;
  return fenced({&d.ec_keys.ev}, s, [&] {
    return launch_ecdsa_sign_keyed(key_id, msgs, moff, mlen, msg_len, n, gate, k.tab.as<uint32_t>(),
                                   k.book.has_live(CORDAHIP_SCHEME_ECDSA_SECP256K1_SHA256),
                                   k.book.has_live(CORDAHIP_SCHEME_ECDSA_SECP256R1_SHA256), sigs, sig_len, status, s);
  });
}

// What the two signing batches differ in: the signature row (64 bytes; a 72-byte DER
// slot) and ECDSA's array of signature lengths (has_len; sig_len: the caller's).
struct SignRows {
  size_t row;
  bool has_len;
  uint8_t* sig_len;
  const char* what;
};
inline SignRows sign_rows(const cordahip_sign_batch*) { return {64, false, nullptr, "sign"}; }
inline SignRows sign_rows(const cordahip_ecdsa_sign_batch* b) {
  return {kEcSignSigBytes, true, b->sig_len, "ECDSA sign"};
}

// A signing call's part of a chunk (keyed_chunks), B cordahip_sign_batch or
// cordahip_ecdsa_sign_batch: the gate bytes in, K11 or K17, the signature rows -- and
// ECDSA's lengths -- out.
template <class B>
struct SignCall {
  Device& d;
  const B* b;
  KeyedStage& st;
  SignRows out;
  bool ensure(const KeyedChunk& c) {
    return st.gate.ensure(c.m) || st.sig_rows.ensure(c.m * out.row) || (out.has_len && st.sig_len.ensure(c.m));
  }
  void pack(const KeyedChunk& c, uint64_t x, uint64_t y) {
    sign_pack_rows(b, c.a, x, y, c.lay, c.poff, st.ids.h.as<uint32_t>(), st.gate.h.as<uint8_t>(),
                   st.msgs.h.as<uint8_t>(), st.msg_off.h.as<uint64_t>(), st.msg_len.h.as<uint32_t>());
  }
  hipError_t enqueue(const KeyedChunk& c) {
    if (b->gate)
      if (const hipError_t e = st.gate.to_device(c.m, c.s)) return e;
    const uint32_t* ids = st.ids.d.as<uint32_t>();
    const uint8_t *msgs = st.msgs.d.as<uint8_t>(), *gate = b->gate ? st.gate.d.as<uint8_t>() : nullptr;
    const uint64_t* moff = c.lay.dense ? nullptr : st.msg_off.d.as<uint64_t>();
    const uint32_t* mlen = c.lay.dense ? nullptr : st.msg_len.d.as<uint32_t>();
    uint8_t *sigs = st.sig_rows.d.as<uint8_t>(), *status = st.status.d.as<uint8_t>();
    std::lock_guard<std::mutex> gs(d.sign_mu);
    return out.has_len
               ? ec_sign_enqueue(d, ids, msgs, moff, mlen, 32, c.m, gate, sigs, st.sig_len.d.as<uint8_t>(), status, c.s)
               : sign_enqueue(d, ids, msgs, moff, mlen, 32, c.m, gate, sigs, status, c.s);
  }
  hipError_t fetch(const KeyedChunk& c) {
    const hipError_t e = st.sig_rows.to_host(c.m * out.row, c.s);
    return e || !out.has_len ? e : st.sig_len.to_host(c.m, c.s);
  }
  void deliver(const KeyedChunk& c) {
    std::memcpy(b->sig + c.a * out.row, st.sig_rows.h.p, c.m * out.row);
    if (out.has_len) std::memcpy(out.sig_len + c.a, st.sig_len.h.p, c.m);
  }
};

// cordahip_sign and cordahip_ecdsa_sign
template <class B>
int sign_impl(cordahip_ctx* ctx, const B* b) {
  const uint64_t n = b->n;
  if (n == 0) return CORDAHIP_SUCCESS;
  const SignRows out = sign_rows(b);
  if (!b->key_id || !b->msg_off || !b->sig || !b->status || (out.has_len && !out.sig_len))
    return CORDAHIP_ERR_INVALID_ARG;
  if (!check_sign_batch(PoolPar{*ctx->host}, b)) return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  if (b->msg_off[0] != b->msg_off[n] && !b->msg) return CORDAHIP_ERR_INVALID_ARG;
  return for_shards(ctx->devs, n, 64, [&](Device& d, uint64_t lo, uint64_t hi) {
    return keyed_chunks(ctx, d, d.sign_stage, b->msg_off, b->status, lo, hi, 1, out.what,
                        SignCall<B>{d, b, d.sign_stage, out});
  });
}

// ---- Ed25519 verification against registered keys (K12, ed25519_vkey.hip) --------
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
  auto& book = d.ec_vkeys.book;
  if (!d.ec_vkeys.tab.p) {
    if (d.ec_vkeys.tab.ensure(ecdsa_vkey_bytes()) != hipSuccess) return CORDAHIP_ERR_OUT_OF_MEMORY;
    book = {};
    if (hipMemsetAsync(d.ec_vkeys.tab.as<uint32_t>() + kEcVkeyRecBase, 0, (kEcVkeyAllWords - kEcVkeyRecBase) * 4,
                       d.stream) != hipSuccess)
      return CORDAHIP_ERR_HIP;
  }
  uint32_t* tab = d.ec_vkeys.tab.as<uint32_t>();
  const bool build_base = !book.table_built(scheme);  // marked built only once the stream has drained below
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
    if (build_base) book.mark_built(scheme);
    if (*decoded) book.take(vkey_slot(key_id), scheme);
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
      [&](Device& d) { (void)clear_slot(d, Registry::kVerify, slot); });  // no device keeps a record of a key the caller never got
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
  if (e == hipSuccess && f == hipSuccess) k.live |= 1ull << vkey_slot(rec.id);
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
      [&](Device& d) { (void)clear_slot(d, Registry::kVerify, slot); });  // no device keeps a record of a key the caller never got
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
  const int rc = clear_slot_on_each_device(ctx, Registry::kVerify, slot);
  if (tracing()) fprintf(stderr, "[cordahip] vkey: key id %u removed (%u live)\n", key_id, reg.count);
  return rc;
}

// The keyed verifiers on stream s (vkey_mu held, device current), each behind its tables'
// previous user and followed by the tables' fence (fenced): Ed25519 (K12) and ECDSA
// (K13). A device without the family's tables yet passes none: every lane is then
// UNKNOWN_KEY.
hipError_t vkey_enqueue(Device& d, const uint32_t* key_id, const uint8_t* sigs, const uint8_t* msgs,
                        const uint64_t* moff, const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* pre,
                        uint32_t flags, uint8_t* status, unsigned long long* verdict, hipStream_t s) {
  return fenced({&d.vkeys.ev}, s, [&] {
    return launch_ed25519_verify_keyed(key_id, sigs, msgs, moff, mlen, msg_len, n, pre, flags,
                                       d.vkeys.tab.as<uint32_t>(), status, verdict, s);
  });
}
hipError_t ec_vkey_enqueue(Device& d, const uint32_t* key_id, const uint8_t* sigs, const uint8_t* sig_len,
                           const uint8_t* msgs, const uint64_t* moff, const uint32_t* mlen, uint32_t msg_len,
                           uint64_t n, const uint8_t* pre, uint32_t flags, uint8_t* status,
                           unsigned long long* verdict, hipStream_t s) {
  const EcVerifyKeys& k = d.ec_vkeys;
  return fenced({&d.ec_vkeys.ev}, s, [&] {
    return launch_ecdsa_verify_keyed(key_id, sigs, sig_len, msgs, moff, mlen, msg_len, n, pre, flags,
                                     k.tab.as<uint32_t>(), k.book.has_live(CORDAHIP_SCHEME_ECDSA_SECP256K1_SHA256),
                                     k.book.has_live(CORDAHIP_SCHEME_ECDSA_SECP256R1_SHA256), status, verdict, s);
  });
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
// previous users, followed by both fences (fenced). A device without an RSA table
// passes none: every lane is then UNKNOWN_KEY.
hipError_t rsa_vkey_enqueue(Device& d, const uint32_t* key_id, const uint8_t* sigs, const uint16_t* sig_len,
                            const uint8_t* msgs, const uint64_t* msg_off, uint32_t msg_len, uint32_t W, uint64_t n,
                            uint32_t flags, uint8_t* status, unsigned long long* verdict, hipStream_t s) {
  RsaWork& w = d.rsa;
  return fenced({&w.ev, &d.rsa_vkeys.ev}, s, [&] {
    return launch_rsa_verify_keyed(d.rsa_vkeys.tab.as<uint32_t>(), key_id, sigs, sig_len, msgs, msg_off, msg_len, W, n,
                                   status, verdict, w.ws.as<uint8_t>(), w.ws.cap / rsa_ws_row_bytes(W) / 64 * 64, flags,
                                   s);
  });
}

// cordahip_rsa_verify_keyed for lanes [lo, hi) on one device, a chunk of
// CORDAHIP_HOST_CHUNK lanes at a time. A chunk's lanes are grouped by their key's width
// class from the context's mirror of the registry (a lane whose id is not live there is
// UNKNOWN_KEY now and is not sent); each class present runs over its rows only, in
// launches of at most kRsaKeyedRows rows through the keyed stage (pack_rows.hpp
// rsa_keyed_pack_rows, one round_trip each) and the statuses go back to their lanes.
// The stage is single: a launch's statuses are read before the next one packs. rsa_mu
// is held for the run (the workspace), outside the stage's lock; the workspace grows
// before vkey_mu is taken, per launch. The verdict words come from the statuses at the
// end of the shard (shards start at multiples of 64 lanes).
constexpr uint64_t kRsaKeyedRows = 1ull << 15;
int rsa_keyed_shard(cordahip_ctx* ctx, Device& d, const cordahip_keyed_sig_batch* b, uint64_t lo, uint64_t hi) {
  KeyedStage& st = d.vkey_stage;
  std::lock_guard<std::mutex> gr(d.rsa_mu);
  ShardRun run(ctx, d, st, 64);
  if (!run.ok) return CORDAHIP_ERR_HIP;
  hipStream_t s = d.stream;
  std::vector<uint64_t> cl[3];  // lanes by class: 64, 96, 128 words
  cordahip_ctx::RsaVkeyMirror mir[kVkeySlots];
  for (uint64_t a = lo; a < hi; a += run.chunk) {
    const uint64_t m = std::min(run.chunk, hi - a);
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
        // the previous launch has drained: growing frees nothing in use
        if (st.msg_off.ensure((rows + 1) * 8)) return CORDAHIP_ERR_OUT_OF_MEMORY;
        uint64_t* mo = st.msg_off.h.as<uint64_t>();
        rsa_keyed_msg_offsets(b, lanes, rows, mo);
        if (st.ids.ensure(rows * 4) || st.sig_rows.ensure(rows * 4 * W) || st.sig_len.ensure(rows * 2) ||
            st.msgs.ensure(std::max<uint64_t>(mo[rows], 16)) || st.status.ensure(rows))
          return CORDAHIP_ERR_OUT_OF_MEMORY;
        run.pool.parallel_for(rows, 256, [&](uint64_t x, uint64_t y) {
          rsa_keyed_pack_rows(b, lanes, W, mo, x, y, st.ids.h.as<uint32_t>(), st.sig_rows.h.as<uint8_t>(),
                              st.sig_len.h.as<uint16_t>(), st.msgs.h.as<uint8_t>());
        });
        bool oom = false;
        const int rc = round_trip(st, rows, s, [&] {
          hipError_t e = st.ids.to_device(rows * 4, s);
          e = e ? e : st.sig_rows.to_device(rows * 4 * W, s);
          e = e ? e : st.sig_len.to_device(rows * 2, s);
          if (mo[rows]) e = e ? e : st.msgs.to_device(mo[rows], s);
          e = e ? e : st.msg_off.to_device((rows + 1) * 8, s);
          if (e == hipSuccess) oom = (e = rsa_ws_grow(d, W, rows)) == hipErrorOutOfMemory;
          if (e) return e;
          std::lock_guard<std::mutex> gv(d.vkey_mu);
          return rsa_vkey_enqueue(d, st.ids.d.as<uint32_t>(), st.sig_rows.d.as<uint8_t>(), st.sig_len.d.as<uint16_t>(),
                                  st.msgs.d.as<uint8_t>(), st.msg_off.d.as<uint64_t>(), 0, W, rows, b->flags,
                                  st.status.d.as<uint8_t>(), nullptr, s);
        });
        if (rc != CORDAHIP_SUCCESS) return oom ? CORDAHIP_ERR_OUT_OF_MEMORY : rc;
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


// The RSA keyed signer on stream s (rsa_mu and sign_mu held, device current, the RSA
// workspace grown for the call: rsa_ws_grow): behind the workspace's and the RSA signer
// table's previous users, followed by both fences (fenced). A device without an RSA
// signer table passes none: every ungated lane is then UNKNOWN_KEY.
hipError_t rsa_sign_enqueue(Device& d, const uint32_t* key_id, const uint8_t* msgs, const uint64_t* msg_off,
                            uint32_t msg_len, const uint8_t* salts, const uint8_t* gate, uint32_t W, uint64_t n,
                            uint8_t* sigs, uint16_t* sig_len, uint8_t* status, hipStream_t s) {
  RsaWork& w = d.rsa;
  return fenced({&w.ev, &d.rsa_keys.ev}, s, [&] {
    return launch_rsa_sign_keyed(d.rsa_keys.tab.as<uint32_t>(), key_id, msgs, msg_off, msg_len, salts, gate, W, n, sigs,
                                 sig_len, status, w.ws.as<uint8_t>(), w.ws.cap / rsa_ws_row_bytes(W), s);
  });
}

// cordahip_rsa_sign for lanes [lo, hi) on one device, rsa_keyed_shard's shape: a chunk of
// CORDAHIP_HOST_CHUNK lanes at a time; a gated lane is SKIPPED and a lane whose id is not
// a live RSA signer's in the context's mirror UNKNOWN_KEY now, neither is sent; the rest
// are grouped by their key's width class and each class present runs over its rows only,
// in launches of at most kRsaSignRows rows through the signer's stage (one round_trip
// each); signatures, lengths and statuses go back to their lanes. rsa_mu is held for the
// run (the workspace), outside the stage's lock; the workspace grows before sign_mu is
// taken, per launch.
constexpr uint64_t kRsaSignRows = 1ull << 14;
int rsa_sign_shard(cordahip_ctx* ctx, Device& d, const cordahip_rsa_sign_batch* b, uint64_t lo, uint64_t hi) {
  KeyedStage& st = d.sign_stage;
  std::lock_guard<std::mutex> gr(d.rsa_mu);
  ShardRun run(ctx, d, st, 1);
  if (!run.ok) return CORDAHIP_ERR_HIP;
  hipStream_t s = d.stream;
  std::vector<uint64_t> cl[3];  // lanes by class: 64, 96, 128 words
  std::vector<cordahip_ctx::RsaVkeyMirror> mir(kSignKeySlots);
  for (uint64_t a = lo; a < hi; a += run.chunk) {
    const uint64_t m = std::min(run.chunk, hi - a);
    const double t0 = now_ms();
    {
      std::lock_guard<std::mutex> gm(ctx->rsa_mirror_mu);
      std::copy(ctx->rsa_sign_mirror, ctx->rsa_sign_mirror + kSignKeySlots, mir.begin());
    }
    for (auto& v : cl) v.clear();
    std::memset(b->sig + a * CORDAHIP_RSA_SIG_SLOT, 0, m * CORDAHIP_RSA_SIG_SLOT);
    for (uint64_t i = a; i < a + m; i++) {
      const uint32_t id = b->key_id[i];
      const auto& k = mir[id & (kSignKeySlots - 1)];
      b->sig_len[i] = 0;
      if (b->gate && b->gate[i]) b->status[i] = CORDAHIP_SIGN_SKIPPED;
      else if (k.words && k.id == id) cl[k.words / 32 - 2].push_back(i);
      else b->status[i] = CORDAHIP_SIGN_UNKNOWN_KEY;
    }
    for (int c = 0; c < 3; c++) {
      const uint32_t W = 64 + 32 * (uint32_t)c;
      for (uint64_t r0 = 0; r0 < cl[c].size(); r0 += kRsaSignRows) {
        const uint64_t rows = std::min<uint64_t>(kRsaSignRows, cl[c].size() - r0);
        const uint64_t* lanes = cl[c].data() + r0;
        // the previous launch has drained: growing frees nothing in use
        if (st.msg_off.ensure((rows + 1) * 8)) return CORDAHIP_ERR_OUT_OF_MEMORY;
        uint64_t* mo = st.msg_off.h.as<uint64_t>();
        mo[0] = 0;
        for (uint64_t r = 0; r < rows; r++) mo[r + 1] = mo[r] + (b->msg_off[lanes[r] + 1] - b->msg_off[lanes[r]]);
        if (st.ids.ensure(rows * 4) || st.salt.ensure(rows * 32) || st.sig_rows.ensure(rows * 4 * W) ||
            st.sig_len.ensure(rows * 2) || st.msgs.ensure(std::max<uint64_t>(mo[rows], 16)) || st.status.ensure(rows))
          return CORDAHIP_ERR_OUT_OF_MEMORY;
        run.pool.parallel_for(rows, 256, [&](uint64_t x, uint64_t y) {
          uint32_t* hid = st.ids.h.as<uint32_t>();
          uint8_t *hs = st.salt.h.as<uint8_t>(), *hm = st.msgs.h.as<uint8_t>();
          for (uint64_t r = x; r < y; r++) {
            const uint64_t i = lanes[r];
            hid[r] = b->key_id[i];
            std::memcpy(hs + r * 32, b->salt + i * 32, 32);
            if (mo[r + 1] != mo[r]) std::memcpy(hm + mo[r], b->msg + b->msg_off[i], mo[r + 1] - mo[r]);
          }
        });
        bool oom = false;
        const int rc = round_trip(st, rows, s, [&] {
          hipError_t e = st.ids.to_device(rows * 4, s);
          e = e ? e : st.salt.to_device(rows * 32, s);
          if (mo[rows]) e = e ? e : st.msgs.to_device(mo[rows], s);
          e = e ? e : st.msg_off.to_device((rows + 1) * 8, s);
          if (e == hipSuccess) oom = (e = rsa_ws_grow(d, W, rows)) == hipErrorOutOfMemory;
          if (e) return e;
          {
            std::lock_guard<std::mutex> gs(d.sign_mu);
            e = rsa_sign_enqueue(d, st.ids.d.as<uint32_t>(), st.msgs.d.as<uint8_t>(), st.msg_off.d.as<uint64_t>(), 0,
                                 st.salt.d.as<uint8_t>(), nullptr, W, rows, st.sig_rows.d.as<uint8_t>(),
                                 st.sig_len.d.as<uint16_t>(), st.status.d.as<uint8_t>(), s);
          }
          e = e ? e : st.sig_rows.to_host(rows * 4 * W, s);
          return e ? e : st.sig_len.to_host(rows * 2, s);
        });
        if (rc != CORDAHIP_SUCCESS) return oom ? CORDAHIP_ERR_OUT_OF_MEMORY : rc;
        const uint8_t *hst = st.status.h.as<uint8_t>(), *hsig = st.sig_rows.h.as<uint8_t>();
        const uint16_t* hl = st.sig_len.h.as<uint16_t>();
        for (uint64_t r = 0; r < rows; r++) {
          b->status[lanes[r]] = hst[r];
          b->sig_len[lanes[r]] = hl[r];
          std::memcpy(b->sig + lanes[r] * CORDAHIP_RSA_SIG_SLOT, hsig + r * 4 * W, 4 * W);
        }
      }
    }
    if (tracing())
      fprintf(stderr, "[cordahip] dev %d RSA sign chunk: %llu lanes (%zu / %zu / %zu by class) in %.2f ms\n", d.id,
              (unsigned long long)m, cl[0].size(), cl[1].size(), cl[2].size(), now_ms() - t0);
  }
  return CORDAHIP_SUCCESS;
}

int rsa_sign_impl(cordahip_ctx* ctx, const cordahip_rsa_sign_batch* b) {
  const uint64_t n = b->n;
  if (n == 0) return CORDAHIP_SUCCESS;
  if (!b->key_id || !b->msg_off || !b->salt || !b->sig || !b->sig_len || !b->status) return CORDAHIP_ERR_INVALID_ARG;
  if (!check_sign_batch(PoolPar{*ctx->host}, b)) return CORDAHIP_ERR_INVALID_ARG;  // before any enqueue
  if (b->msg_off[0] != b->msg_off[n] && !b->msg) return CORDAHIP_ERR_INVALID_ARG;
  return for_shards(ctx->devs, n, 64,
                    [&](Device& d, uint64_t lo, uint64_t hi) { return rsa_sign_shard(ctx, d, b, lo, hi); });
}

// A device's cumulative counters of routed lanes: route_tot of the family's key table
// `keys` (K14: Device::vkeys, K15: Device::ec_vkeys, K20: Device::rsa_vkeys), written by kernels the table's
// fence follows.
template <class Keys>
int route_stats(cordahip_ctx* ctx, int device, Keys Device::*keys, uint64_t* keyed_lanes, uint64_t* generic_lanes) {
  Device* d = dev_at(ctx, device);
  if (!d || !keyed_lanes || !generic_lanes) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    const Keys& k = d->*keys;
    std::lock_guard<std::mutex> g(d->vkey_mu);
    uint64_t tot[2] = {0, 0};
    if (k.route_tot.p) {  // else: no routed enqueue of this family on this device yet
      // every routed enqueue's partition pass is followed by the table's fence
      if (hipSetDevice(d->id) != hipSuccess || k.ev.sync() != hipSuccess ||
          hipMemcpy(tot, k.route_tot.p, sizeof tot, hipMemcpyDeviceToHost) != hipSuccess)
        return CORDAHIP_ERR_HIP;
    }
    *keyed_lanes = tot[0];
    *generic_lanes = tot[1];
    return CORDAHIP_SUCCESS;
  });
}
// a routing switch (Device::route_on, Device::ec_route_on, Device::rsa_route_on, Device::sig_route_on) on
// every device
int set_routing(cordahip_ctx* ctx, std::atomic<uint32_t> Device::*sw, uint32_t on) {
  if (!ctx) return CORDAHIP_ERR_INVALID_ARG;
  for (auto& dp : ctx->devs) ((*dp).*sw).store(on ? 1u : 0u);
  return CORDAHIP_SUCCESS;
}

// a *_keyed_device entry point that needs one lock: device_call under `mu`, guarded
template <class F>
int locked_device_call(Device& d, std::mutex& mu, void* hip_stream, F&& enqueue) {
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(mu);
    return device_call(d, hip_stream, enqueue);
  });
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
  return submit(ctx, ticket, sign_impl<cordahip_sign_batch>, batch);
}

int cordahip_ed25519_sign_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_msgs,
                                       uint32_t msg_len, uint64_t n, const void* d_gate, void* d_sigs,
                                       void* d_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (n && (!d_key_id || !d_sigs || !d_status || (msg_len && !d_msgs)))) return CORDAHIP_ERR_INVALID_ARG;
  if (misaligned(d_sigs, 16) || misaligned(d_key_id, 4) || (msg_len == 32 && misaligned(d_msgs, 16)))
    return CORDAHIP_ERR_INVALID_ARG;
  return locked_device_call(*d, d->sign_mu, hip_stream, [&](hipStream_t s) {
    return sign_enqueue(*d, ptr<uint32_t>(d_key_id), ptr<uint8_t>(d_msgs), nullptr, nullptr, msg_len, n,
                        ptr<uint8_t>(d_gate), ptr<uint8_t>(d_sigs), ptr<uint8_t>(d_status), s);
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
  return guarded([&] { return sign_impl(ctx, batch); });
}

int cordahip_ecdsa_sign_submit(cordahip_ctx* ctx, const cordahip_ecdsa_sign_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, sign_impl<cordahip_ecdsa_sign_batch>, batch);
}

int cordahip_ecdsa_sign_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_msgs,
                                     uint32_t msg_len, uint64_t n, const void* d_gate, void* d_sigs,
                                     void* d_sig_len, void* d_status, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (n && (!d_key_id || !d_sigs || !d_sig_len || !d_status || (msg_len && !d_msgs))))
    return CORDAHIP_ERR_INVALID_ARG;
  if (misaligned(d_sigs, 4) || misaligned(d_key_id, 4)) return CORDAHIP_ERR_INVALID_ARG;
  return locked_device_call(*d, d->sign_mu, hip_stream, [&](hipStream_t s) {
    return ec_sign_enqueue(*d, ptr<uint32_t>(d_key_id), ptr<uint8_t>(d_msgs), nullptr, nullptr, msg_len, n,
                           ptr<uint8_t>(d_gate), ptr<uint8_t>(d_sigs), ptr<uint8_t>(d_sig_len),
                           ptr<uint8_t>(d_status), s);
  });
}

int cordahip_signer_add_rsa(cordahip_ctx* ctx, const cordahip_rsa_private_key* key, uint32_t* key_id,
                            uint8_t* key_status, uint8_t modulus[512], uint32_t* modulus_len) {
  if (!ctx || !key || !key_id || !key_status || !modulus || !modulus_len) return CORDAHIP_ERR_INVALID_ARG;
  if (!key->p || !key->q || !key->dp || !key->dq || !key->qinv) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return rsa_signer_add_impl(ctx, key, key_id, key_status, modulus, modulus_len); });
}

int cordahip_rsa_sign(cordahip_ctx* ctx, const cordahip_rsa_sign_batch* batch) {
  if (!ctx || !batch) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&] { return rsa_sign_impl(ctx, batch); });
}

int cordahip_rsa_sign_submit(cordahip_ctx* ctx, const cordahip_rsa_sign_batch* batch, uint64_t* ticket) {
  return submit(ctx, ticket, rsa_sign_impl, batch);
}

int cordahip_rsa_sign_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_msgs,
                                   uint32_t msg_len, const void* d_salts, uint32_t mod_words, uint64_t n,
                                   const void* d_gate, void* d_sigs, void* d_sig_len, void* d_status,
                                   void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (mod_words != 64 && mod_words != 96 && mod_words != 128) ||
      (n && (!d_key_id || !d_salts || !d_sigs || !d_sig_len || !d_status || (msg_len && !d_msgs))))
    return CORDAHIP_ERR_INVALID_ARG;
  if (misaligned(d_key_id, 4) || misaligned(d_sig_len, 2)) return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(d->rsa_mu);
    return device_call(
        *d, hip_stream, [&] { return rsa_ws_grow(*d, mod_words, n); },
        [&](hipStream_t s) {
          std::lock_guard<std::mutex> gs(d->sign_mu);
          return rsa_sign_enqueue(*d, ptr<uint32_t>(d_key_id), ptr<uint8_t>(d_msgs), nullptr, msg_len,
                                  ptr<uint8_t>(d_salts), ptr<uint8_t>(d_gate), mod_words, n, ptr<uint8_t>(d_sigs),
                                  ptr<uint16_t>(d_sig_len), ptr<uint8_t>(d_status), s);
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

int cordahip_vkey_set_routing(cordahip_ctx* ctx, uint32_t on) { return set_routing(ctx, &Device::route_on, on); }

int cordahip_vkey_route_stats(cordahip_ctx* ctx, int device, uint64_t* keyed_lanes, uint64_t* generic_lanes) {
  return route_stats(ctx, device, &Device::vkeys, keyed_lanes, generic_lanes);
}

int cordahip_vkey_set_routing_ecdsa(cordahip_ctx* ctx, uint32_t on) {
  return set_routing(ctx, &Device::ec_route_on, on);
}

int cordahip_vkey_route_stats_ecdsa(cordahip_ctx* ctx, int device, uint64_t* keyed_lanes, uint64_t* generic_lanes) {
  return route_stats(ctx, device, &Device::ec_vkeys, keyed_lanes, generic_lanes);
}

int cordahip_vkey_set_routing_rsa(cordahip_ctx* ctx, uint32_t on) {
  return set_routing(ctx, &Device::rsa_route_on, on);
}

int cordahip_vkey_route_stats_rsa(cordahip_ctx* ctx, int device, uint64_t* keyed_rows, uint64_t* generic_rows) {
  return route_stats(ctx, device, &Device::rsa_vkeys, keyed_rows, generic_rows);
}

// K24: whether the mixed device calls (runtime.cpp sig_device_enqueue) consult the three switches above
int cordahip_vkey_set_routing_device(cordahip_ctx* ctx, uint32_t on) {
  return set_routing(ctx, &Device::sig_route_on, on);
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
  if (misaligned(d_sigs, 16) || misaligned(d_key_id, 4) || misaligned(d_verdict, 8) ||
      (msg_len == 32 && misaligned(d_msgs, 16)))
    return CORDAHIP_ERR_INVALID_ARG;
  return locked_device_call(*d, d->vkey_mu, hip_stream, [&](hipStream_t s) {
    return vkey_enqueue(*d, ptr<uint32_t>(d_key_id), ptr<uint8_t>(d_sigs), ptr<uint8_t>(d_msgs), nullptr, nullptr,
                        msg_len, n, nullptr, 0u, ptr<uint8_t>(d_status), ptr<unsigned long long>(d_verdict), s);
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
  if (misaligned(d_key_id, 4) || misaligned(d_verdict, 8)) return CORDAHIP_ERR_INVALID_ARG;
  return locked_device_call(*d, d->vkey_mu, hip_stream, [&](hipStream_t s) {
    return ec_vkey_enqueue(*d, ptr<uint32_t>(d_key_id), ptr<uint8_t>(d_sigs), ptr<uint8_t>(d_sig_len),
                           ptr<uint8_t>(d_msgs), nullptr, nullptr, msg_len, n, nullptr, 0u, ptr<uint8_t>(d_status),
                           ptr<unsigned long long>(d_verdict), s);
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
  if (misaligned(d_key_id, 4) || misaligned(d_sig_len, 2) || misaligned(d_verdict, 8))
    return CORDAHIP_ERR_INVALID_ARG;
  return guarded([&]() -> int {
    std::lock_guard<std::mutex> g(d->rsa_mu);
    return device_call(
        *d, hip_stream, [&] { return rsa_ws_grow(*d, mod_words, n); },
        [&](hipStream_t s) {
          std::lock_guard<std::mutex> gv(d->vkey_mu);
          return rsa_vkey_enqueue(*d, ptr<uint32_t>(d_key_id), ptr<uint8_t>(d_sigs), ptr<uint16_t>(d_sig_len),
                                  ptr<uint8_t>(d_msgs), nullptr, msg_len, mod_words, n, 0u, ptr<uint8_t>(d_status),
                                  ptr<unsigned long long>(d_verdict), s);
        });
  });
}

int cordahip_rsa_public_op_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_in,
                                        uint32_t mod_words, uint64_t n, void* d_out, void* hip_stream) {
  Device* d = dev_at(ctx, device);
  if (!d || (mod_words != 64 && mod_words != 96 && mod_words != 128) || (n && (!d_key_id || !d_in || !d_out)))
    return CORDAHIP_ERR_INVALID_ARG;
  if (misaligned(d_key_id, 4) || misaligned(d_in, 4) || misaligned(d_out, 4)) return CORDAHIP_ERR_INVALID_ARG;
  // no workspace: the table's lock and fence alone
  return locked_device_call(*d, d->vkey_mu, hip_stream, [&](hipStream_t s) {
    return fenced({&d->rsa_vkeys.ev}, s, [&] {
      return launch_rsa_public_op_keyed(d->rsa_vkeys.tab.as<uint32_t>(), ptr<uint32_t>(d_key_id),
                                        ptr<uint32_t>(d_in), mod_words, n, ptr<uint32_t>(d_out), s);
    });
  });
}

}  // extern "C"
