// libcordahip's internal runtime types (not ABI): per-device state and what it
// owns (buffers, fences, events, streams), the ticket pool, the host thread pool
// and the enqueue helpers (runtime.cpp) shared by cordahip.cpp (C-ABI, tx /
// stream / device paths), keyed.cpp (registered keys), commit_api.cpp (the commit
// log) and host_batch.cpp (the generic CSR signature batch).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cstdlib>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <future>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/cordahip.h"
#include "commit_core.hpp"
#include "key_slots.hpp"
#include "notary_rows.hpp"
#include "numa_place.hpp"

namespace cordahip {
// commit_log.hip (K16): a commit call's launches (clamp, pre-pass, the claim / win /
// lose rounds, in-order sweep, report; scratch: commit_scratch_bytes(ntx, n_refs);
// entries: the log's entry counter), the
// unfiltered lookup, the load (claim + insert; counters: entries, rows already present) and
// the rehash of every entry into a new, zeroed table
size_t commit_scratch_bytes(uint64_t ntx, uint64_t n_refs);
hipError_t launch_commit_inputs(const commit::Table& T, commit::Batch B, uint64_t n_refs, uint64_t base, void* scratch,
                                unsigned long long* entries, hipStream_t s);
hipError_t launch_commit_lookup(const commit::Table& T, const uint32_t* refs, uint64_t n, uint8_t* present,
                                uint32_t* by, hipStream_t s);
size_t commit_load_scratch_bytes(uint64_t n);
hipError_t launch_commit_load(const commit::Table& T, const uint32_t* rows, uint64_t n, void* scratch,
                              unsigned long long* counters, hipStream_t s);
hipError_t launch_commit_rehash(const commit::Table& from, const commit::Table& to, hipStream_t s);
// the revoke (mark + per-cluster repair; counters: entries, entries removed by this call)
// and the export of the live entries with a sequence number >= since_seq (*total: how many)
size_t commit_revoke_scratch_bytes(uint64_t n);
hipError_t launch_commit_revoke(const commit::Table& T, const uint32_t* rows, uint64_t n, uint8_t* revoked,
                                void* scratch, unsigned long long* counters, hipStream_t s);
hipError_t launch_commit_export(const commit::Table& T, uint64_t since_seq, uint32_t* rows, uint64_t* seq,
                                uint64_t cap, unsigned long long* total, hipStream_t s);
hipError_t launch_ed25519_btable(uint32_t* tab, hipStream_t s);
size_t ed25519_btable_bytes();
hipError_t launch_ed25519_verify(const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                 uint64_t n, const uint32_t* btab, const uint8_t* pre_status, uint8_t* status,
                                 unsigned long long* verdict, uint32_t* ws, uint64_t ws_lanes, uint32_t flags,
                                 hipStream_t s,
                                 const std::function<hipError_t()>* before_msgs = nullptr);
size_t ed25519_ws_lane_bytes();
hipError_t launch_ed25519_sign(const uint8_t* seeds, const uint8_t* msgs, uint32_t msg_len, uint64_t n,
                               const uint32_t* btab, uint8_t* pubs, uint8_t* sigs, hipStream_t s);
// ed25519_sign.hip (K11): the comb table [d 16^j]B, the key table's expansion
// kernel (the seed is in the table's scratch words; the public key comes back
// there: ed25519_comb.hpp kSignSeedWord / kSignPubWord) and the keyed signer
// (moff / mlen non-null: per-lane message offsets and lengths, else dense rows)
size_t ed25519_comb_bytes();
size_t ed25519_keytab_bytes();
hipError_t launch_ed25519_comb(uint32_t* tab, hipStream_t s);
hipError_t launch_ed25519_key_expand(uint32_t* keytab, uint32_t key_id, const uint32_t* comb, hipStream_t s);
hipError_t launch_ed25519_sign_keyed(const uint32_t* key_id, const uint8_t* msgs, const uint64_t* moff,
                                     const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* gate,
                                     const uint32_t* keytab, const uint32_t* comb, uint8_t* sigs, uint8_t* status,
                                     hipStream_t s);
// ecdsa_sign_keyed.hip (K17, in ecdsa.hip's unit): a curve's comb table [d 16^j]G built
// in the ECDSA signer's table, a key added (d is in the table's scratch words, the
// answer and Q = [d]G come back there: ecdsa_sign_core.hpp kEcSignKeyWord /
// kEcSignOutWord) and the keyed signer (messages and gate as for
// launch_ed25519_sign_keyed; 72-byte DER slots with lengths out; live_k1 / live_r1: the
// curves that have a live signer key on the device)
size_t ecdsa_signtab_bytes();
hipError_t launch_ecdsa_sign_comb(uint32_t* tab, uint32_t scheme, hipStream_t s);
hipError_t launch_ecdsa_signer_add(uint32_t* tab, uint32_t scheme, uint32_t key_id, hipStream_t s);
hipError_t launch_ecdsa_sign_keyed(const uint32_t* key_id, const uint8_t* msgs, const uint64_t* moff,
                                   const uint32_t* mlen, uint32_t msg_len, uint64_t n, const uint8_t* gate,
                                   const uint32_t* tab, bool live_k1, bool live_r1, uint8_t* sigs, uint8_t* sig_len,
                                   uint8_t* status, hipStream_t s);
// ed25519_vkey.hip (K12): a verification key's record and window table built in the
// device's key table (the 32 key bytes are in the table's scratch words, the decode
// verdict comes back there: ed25519_vkey.hpp kVkeyKeyWord / kVkeyOkWord) and the keyed
// verifier (moff / mlen non-null: per-lane message offsets and lengths, else dense
// rows; pre: optional per-lane statuses decided by the host; flags: CORDAHIP_FLAG_IS_VALID)
size_t ed25519_vkey_bytes();
hipError_t launch_ed25519_vkey_build(uint32_t* vtab, uint32_t key_id, hipStream_t s);
hipError_t launch_ed25519_vkey_base(uint32_t* vtab, hipStream_t s);  // the table of B, once per device
hipError_t launch_ed25519_verify_keyed(const uint32_t* key_id, const uint8_t* sigs, const uint8_t* msgs,
                                       const uint64_t* moff, const uint32_t* mlen, uint32_t msg_len, uint64_t n,
                                       const uint8_t* pre, uint32_t flags, const uint32_t* vtab, uint8_t* status,
                                       unsigned long long* verdict, hipStream_t s);
// K14 (ed25519_route.hip, ed25519_route.hpp): routed Ed25519 batches. The partition
// pass fills `scratch` (ed25519_route_scratch_bytes(n): route ids, the keyed and the
// generic list, their counts; at least that large) and adds to the device's cumulative counters; the
// indexed instances of K12 and K1 run over the lists, their lane counts read on the
// device; the verdict words are gathered from the statuses afterwards.
size_t ed25519_route_scratch_bytes(uint64_t n);  // a capacity: powers of two from a floor
uint64_t ed25519_route_max_lanes();              // larger batches are not routed (32-bit lane indices)
// count (K24): null, or the device's word holding how many of the n rows to partition
// (clipped to n on the device); rows past it enter neither list.
hipError_t launch_ed25519_route(const uint8_t* keys, uint64_t n, const uint32_t* vtab, uint32_t* scratch,
                                unsigned long long* totals, hipStream_t s, const uint32_t* count = nullptr);
hipError_t launch_ed25519_verify_keyed_idx(const uint32_t* scratch, uint64_t lanes, const uint8_t* sigs,
                                           const uint8_t* msgs, uint32_t msg_len, const uint8_t* pre, uint32_t flags,
                                           const uint32_t* vtab, uint8_t* status, hipStream_t s);
constexpr uint64_t kEdIdxLayoutOfN = ~0ull;  // launch_ed25519_verify_idx: the scratch is laid out for n lanes
hipError_t launch_ed25519_verify_idx(const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs, uint32_t msg_len,
                                     uint64_t n, const uint32_t* btab, const uint8_t* pre_status, uint8_t* status,
                                     uint32_t* ws, uint64_t ws_lanes, uint32_t flags, const uint32_t* scratch,
                                     hipStream_t s, uint64_t layout_lanes = kEdIdxLayoutOfN);
hipError_t launch_ed25519_status_verdict(const uint8_t* status, uint64_t n, unsigned long long* verdict,
                                         hipStream_t s);
hipError_t launch_sha256_leaves(const uint8_t* bytes, const uint64_t* off, uint64_t nleaves, uint32_t* hashes,
                                hipStream_t s);
hipError_t launch_merkle_root(uint32_t* hashes, const uint64_t* tx_leaf_off, uint64_t ntx, uint8_t* txid,
                              uint8_t* tx_status, hipStream_t s, const uint8_t* item_status = nullptr,
                              uint8_t* map_txid = nullptr, uint8_t* map_status = nullptr);
hipError_t launch_gather_txid(const uint8_t* txid, const uint64_t* tx_sig_off, uint64_t ntx, uint8_t* msgs,
                              hipStream_t s);
hipError_t launch_store_to_host(const void* src, void* dst, uint64_t n, hipStream_t s);
hipError_t tx_set_id_priority(uint32_t on);  // the id kernels' raised wave priority (current device)
hipError_t kryo_set_priority(uint32_t on);   // the same for the Kryo encoder's kernels
// kryo_device.hip: the GPU Kryo leaf encoder (shapes, templates, sizes, scan, writes)
size_t kryo_fixed_scratch_bytes();                     // shape table, records, templates (persistent per device)
size_t kryo_direct_ws_bytes(uint64_t writers);         // the direct encoder's level buffers
hipError_t kryo_scan_bytes(size_t& bytes, uint64_t n1, hipStream_t s);
hipError_t kryo_clear(uint8_t* fixed, hipStream_t s);  // empty the shape table (and the template arena)
// device: [templates in the arena, table slots in use, misses of buffer set 0, of set 1]
// (each set's since its kryo_reset_misses)
const uint32_t* kryo_usage_src(uint8_t* fixed);
constexpr size_t kKryoUsageBytes = 16;
hipError_t kryo_reset_misses(uint8_t* fixed, uint32_t set, hipStream_t s);
uint32_t kryo_clear_threshold_slots();
uint32_t kryo_clear_threshold_templates();
// data_base != nullptr: items' `data` are offsets into data_len bytes at data_base.
// templates_only: the steady-state chain -- no new shapes built, no direct encoder;
// an item that would need either is a miss (counted, its leaf not written, status
// kKryoMiss) and the caller redoes the batch with templates_only false.
constexpr uint8_t kKryoMiss = 4;
hipError_t launch_kryo_encode(const cordahip_kryo_item* items, const uint8_t* data_base, uint64_t data_len,
                              uint64_t n, uint32_t group, uint8_t* fixed,
                              uint32_t* item_slot, uint32_t* direct, uint64_t* sizes, uint64_t* off, uint8_t* out,
                              uint64_t cap, uint8_t* status, uint8_t* dws, uint64_t dwriters, void* scan_temp,
                              size_t scan_bytes, hipStream_t s, bool templates_only = false, uint32_t set = 0);
// the shape pass alone (sizes, item_slot, statuses; kCMiss counts misses)
hipError_t launch_kryo_shape(const cordahip_kryo_item* items, const uint8_t* data_base, uint64_t data_len, uint64_t n,
                             uint32_t group, uint8_t* fixed, uint32_t* item_slot, uint32_t* direct, uint64_t* sizes,
                             uint8_t* status, hipStream_t s, bool templates_only, uint32_t set = 0);
// SHA-256 of every item's leaf straight from its template (after a templates-only shape
// pass): hashes[n][8] big-endian words, zero for items with a nonzero status
hipError_t launch_kryo_shape_hash(const cordahip_kryo_item* d_items, const uint8_t* data_base, uint64_t data_len,
                                  uint64_t n, uint32_t group, uint8_t* fixed, uint8_t* status, uint32_t* hashes,
                                  hipStream_t s, uint32_t set);
hipError_t launch_kryo_hash(const cordahip_kryo_item* items, const uint8_t* data_base, uint64_t data_len, uint64_t n,
                            uint32_t group, uint8_t* fixed, const uint32_t* item_slot, const uint64_t* sizes,
                            const uint8_t* status, uint32_t* hashes, hipStream_t s);
// the device hash chain (no misses, no leaf bytes): shapes -> build -> tsize ->
// kryo_hash -> kryo_dhash (the direct encoder into a SHA-256 sink); hashes[n][8]
// big-endian words, zero for an item the encoder rejects (status 1)
hipError_t launch_kryo_hash_chain(const cordahip_kryo_item* items, const uint8_t* data_base, uint64_t data_len,
                                  uint64_t n, uint32_t group, uint8_t* fixed, uint32_t* item_slot, uint32_t* direct,
                                  uint64_t* sizes, uint8_t* status, uint32_t* hashes, uint8_t* dws, uint64_t dwriters,
                                  hipStream_t s);
hipError_t launch_gather_rows32(const uint8_t* txid, const uint32_t* idx, uint64_t n, uint8_t* rows, hipStream_t s);
hipError_t launch_tx_reduce(uint8_t* sig_status, const uint64_t* tx_sig_off, uint64_t ntx, int64_t* first_bad,
                            uint8_t* tx_status, hipStream_t s);
// K9 (tx.hip): required-signer coverage, one lane per transaction; `c` holds device pointers.
// sig_scheme nullptr: all Ed25519; sig_key_off nullptr: dense 32-byte key rows
hipError_t launch_tx_cover(const cordahip_cover& c, uint64_t ntx, uint8_t* tx_status, const uint64_t* tx_sig_off,
                           const uint8_t* sig_scheme, const uint8_t* sig_key, const uint64_t* sig_key_off,
                           uint64_t* stack, hipStream_t s);
hipError_t launch_pmt_verify(const uint32_t* leaf_hashes, const uint64_t* tx_leaf_off, const uint8_t* tok,
                             const uint8_t* tok_hash, const uint64_t* tx_tok_off, const uint8_t* root, uint64_t ntx,
                             uint32_t* stack, uint8_t* tx_status, hipStream_t s,
                             const uint8_t* bad_component = nullptr);
// K21 (kryo_device.hip): a notary tear-off's leaf hashes from typed rows. R holds device
// pointers (tw_flags nullptr: no windows). tx_leaf_off [ntx+1], hashes [(n_refs + ntx) * 8]
// words as K6 reads them, leaf_hash (may be nullptr) the same hashes as bytes, tw_from /
// tw_until / bad [ntx]: the windows as cordahip_commit_batch takes them and the
// transactions whose window row is no valid item.
hipError_t launch_notary_leaves(const NotaryRows& R, uint64_t* tx_leaf_off, uint32_t* hashes, uint8_t* leaf_hash,
                                int64_t* tw_from, int64_t* tw_until, uint8_t* bad, hipStream_t s);
// gate[t] = verify[t] != OK or caller_gate[t] (may be nullptr) set; status[t] = verify[t] if not OK, else commit[t]
hipError_t launch_notary_gate(const uint8_t* verify, const uint8_t* caller_gate, uint8_t* gate, uint64_t ntx,
                              hipStream_t s);
hipError_t launch_notary_status(const uint8_t* verify, const uint8_t* commit, uint8_t* status, uint64_t ntx,
                                hipStream_t s);
// K22 (txcomp_inputs.hip): a component batch's STATE_REF items as commit rows and its
// TIME_WINDOW items as window bounds (txcomp_inputs_core.hpp); tx_status may be nullptr
hipError_t launch_txcomp_inputs(const cordahip_kryo_item* d_items, uint64_t n_items, const uint8_t* d_payload,
                                uint64_t payload_len, const uint64_t* d_tx_item_off, uint64_t ntx,
                                const uint8_t* d_tx_status, uint32_t* d_refs, uint64_t ref_cap, uint64_t* d_tx_ref_off,
                                int64_t* d_tw_from, int64_t* d_tw_until, uint8_t* d_gate, hipStream_t s);
// K10 (tx.hip): up = 2 * nleaves hashes, has = 3 * nleaves bytes of workspace (pmt_core.hpp)
hipError_t launch_pmt_build(const uint32_t* hashes, const uint64_t* tx_leaf_off, uint64_t ntx, const uint8_t* include,
                            const uint64_t* tx_tok_off, uint64_t ntok, uint32_t* up, uint8_t* has, uint8_t* txid,
                            uint8_t* tok, uint8_t* tok_hash, uint64_t* tx_ntok, uint8_t* tx_status, hipStream_t s);
size_t ecdsa_gtable_bytes();
hipError_t launch_ecdsa_gtables(uint32_t* k1, uint32_t* r1, hipStream_t s);
hipError_t launch_ecdsa_verify(const uint8_t* scheme, const uint8_t* keys, const uint8_t* key_len,
                               const uint8_t* sigs, const uint8_t* sig_len, const uint8_t* msgs,
                               const uint64_t* msg_off, uint32_t msg_len, uint64_t n, const uint32_t* gk1,
                               const uint32_t* gr1, const uint8_t* pre_status, uint8_t* status,
                               unsigned long long* verdict, unsigned int* counters6, unsigned int* perm,
                               uint32_t* ws, uint64_t ws_slots, uint32_t flags, hipStream_t s);
size_t ecdsa_ws_slot_bytes();
// ecdsa_vkey.hip (K13): a registered ECDSA key's record and window table built in the
// device's table (the SEC1 bytes are in the table's scratch words, the decode verdict
// comes back there: ecdsa_vkey.hpp kEcVkeyKeyWord / kEcVkeyOkWord; slot >= 64: the
// curve's base-point table) and the keyed verifier (72-byte DER slots with lengths;
// messages, pre and flags as for launch_ed25519_verify_keyed; live_k1 / live_r1: the
// curves that have a live key on the device)
size_t ecdsa_vkey_bytes();
hipError_t launch_ecdsa_vkey_build(uint32_t* vtab, uint32_t scheme, uint32_t slot, uint32_t key_id, uint32_t key_len,
                                   hipStream_t s);
hipError_t launch_ecdsa_verify_keyed(const uint32_t* key_id, const uint8_t* sigs, const uint8_t* sig_len,
                                     const uint8_t* msgs, const uint64_t* moff, const uint32_t* mlen, uint32_t msg_len,
                                     uint64_t n, const uint8_t* pre, uint32_t flags, const uint32_t* vtab,
                                     bool live_k1, bool live_r1, uint8_t* status, unsigned long long* verdict,
                                     hipStream_t s);
// K15 (ecdsa_route.hip, ecdsa_route.hpp): routed ECDSA batches. The route pass fills
// `scratch` (ecdsa_route_scratch_bytes(n): the gathered records and route ids; at
// least that large), the seven class counts and cursors in `counters` (64 bytes) and
// perm[n] -- the generic list first, then each curve's keyed run -- and adds to the
// device's cumulative counters; the indexed instances of K13 and K2 run over the
// lists, their lane counts read on the device. count (K24): as launch_ed25519_route's;
// rows past it enter no class.
size_t ecdsa_route_scratch_bytes(uint64_t n);  // a capacity: powers of two from a floor
uint64_t ecdsa_route_max_lanes();              // larger batches are not routed (32-bit lane indices)
hipError_t launch_ecdsa_route(const uint8_t* scheme, const uint8_t* keys, const uint8_t* key_len, uint64_t n,
                              const uint32_t* vtab, uint32_t* scratch, unsigned int* counters, unsigned int* perm,
                              unsigned long long* totals, hipStream_t s, const uint32_t* count = nullptr);
hipError_t launch_ecdsa_verify_keyed_idx(const uint32_t* scratch, const unsigned int* perm,
                                         const unsigned int* counters, uint64_t n, const uint8_t* sigs,
                                         const uint8_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off,
                                         uint32_t msg_len, const uint8_t* pre, uint32_t flags, const uint32_t* vtab,
                                         bool live_k1, bool live_r1, uint8_t* status, hipStream_t s);
hipError_t launch_ecdsa_verify_routed(const uint8_t* scheme, const uint8_t* keys, const uint8_t* key_len,
                                      const uint8_t* sigs, const uint8_t* sig_len, const uint8_t* msgs,
                                      const uint64_t* msg_off, uint32_t msg_len, uint64_t n, const uint32_t* gk1,
                                      const uint32_t* gr1, const uint8_t* pre_status, uint8_t* status,
                                      unsigned long long* verdict, const unsigned int* counters,
                                      const unsigned int* perm, uint32_t* ws, uint64_t ws_slots, uint32_t flags,
                                      hipStream_t s);
// rsa.hip: rows of W = 64 / 96 / 128 little-endian words, one width per launch
uint32_t rsa_group_lanes();  // lanes that share one signature in rsa_modexp_kernel
hipError_t launch_rsa_public_op(const uint32_t* mod, const uint32_t* exp, const uint32_t* in, uint32_t W, uint64_t n,
                                uint32_t* out, hipStream_t s);
size_t rsa_ws_row_bytes(uint32_t W);
// msg_off != nullptr: CSR messages (msg_off[n + 1] into msgs), else n * msg_len dense;
// ws: ws_rows * rsa_ws_row_bytes(W) bytes, the launches loop over it
hipError_t launch_rsa_pss_verify(const uint32_t* mod, const uint32_t* exp, const uint8_t* sigs,
                                 const uint16_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off,
                                 uint32_t msg_len, uint32_t W, uint64_t n, const uint8_t* pre, uint8_t* status,
                                 unsigned long long* verdict, uint8_t* ws, uint64_t ws_rows, uint32_t flags,
                                 hipStream_t s);
// rsa_vkey.hip (K18, in rsa.hip's unit): the same against registered keys. vtab: the
// device's RSA key table (rsa_vkey.hpp: rsa_vkey_bytes(); null: no key was ever added,
// every row is unknown); key_id[n]; one width class per launch. The raw op gives a zero
// row for a key that is not live in class W or in >= n; the verifier answers
// UNKNOWN_KEY first, then the statuses of launch_rsa_pss_verify.
size_t rsa_vkey_bytes();
hipError_t launch_rsa_public_op_keyed(const uint32_t* vtab, const uint32_t* key_id, const uint32_t* in, uint32_t W,
                                      uint64_t n, uint32_t* out, hipStream_t s);
hipError_t launch_rsa_verify_keyed(const uint32_t* vtab, const uint32_t* key_id, const uint8_t* sigs,
                                   const uint16_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off,
                                   uint32_t msg_len, uint32_t W, uint64_t n, uint8_t* status,
                                   unsigned long long* verdict, uint8_t* ws, uint64_t ws_rows, uint32_t flags,
                                   hipStream_t s);
// rsa_route.hip (K20, in rsa.hip's unit): one launch of a routed batch in three parts --
// the prep; the counts cleared, the route pass (rsa_route.hpp) and K18's exponentiation
// over the keyed list; K8's over the generic list and the check -- so that the caller
// holds the key table's lock around the middle one only. m rows from row lo, at most
// rsa_launch_rows(ws_rows); scratch: rsa_route_scratch_bytes(cap_rows), cap_rows >= m;
// totals: the device's cumulative (keyed, generic) row counters. routed false in the
// tail: the middle part did not run, K8's kernel takes every row as in an unrouted launch.
// count (K24; null for the dense calls): the batch's rows are known on the device only
// and m is the host's bound; the head writes the launch's rows, clipped to m, to
// *launch_count, which the other two parts take (iota: row j of the list is row j, at
// least m words, for a tail that is not routed).
size_t rsa_route_scratch_bytes(uint64_t cap_rows);
uint64_t rsa_launch_rows(uint64_t ws_rows);
hipError_t launch_rsa_routed_head(const uint32_t* mod, const uint32_t* exp, const uint8_t* sigs,
                                  const uint16_t* sig_len, const uint64_t* msg_off, uint32_t msg_len, uint32_t W,
                                  uint64_t lo, uint64_t m, const uint8_t* pre, uint8_t* ws, uint64_t ws_rows,
                                  uint32_t flags, hipStream_t s, const unsigned int* count = nullptr,
                                  unsigned int* launch_count = nullptr);
hipError_t launch_rsa_routed_keyed(const uint32_t* mod, const uint32_t* exp, uint32_t W, uint64_t lo, uint64_t m,
                                   const uint32_t* vtab, uint8_t* ws, uint64_t ws_rows, uint32_t* scratch,
                                   uint64_t cap_rows, unsigned long long* totals, hipStream_t s,
                                   const unsigned int* launch_count = nullptr);
hipError_t launch_rsa_routed_tail(const uint32_t* mod, const uint32_t* exp, const uint8_t* msgs,
                                  const uint64_t* msg_off, uint32_t msg_len, uint32_t W, uint64_t lo, uint64_t m,
                                  uint8_t* status, unsigned long long* verdict, uint8_t* ws, uint64_t ws_rows,
                                  const uint32_t* scratch, uint64_t cap_rows, bool routed, hipStream_t s,
                                  const unsigned int* launch_count = nullptr,
                                  const unsigned int* iota = nullptr);
// rsa_sign_keyed.hip (K19, in rsa.hip's unit): RSASSA-PSS signatures with registered
// private keys. stab: the device's RSA signer table (rsa_sign.hpp: rsa_signtab_bytes();
// null: no key was ever added, every ungated row is unknown); key_id[n], salts[n * 32],
// gate[n] or null; one width class per launch; sigs: 4 W-byte slots, sig_len uint16[n].
// ws as for launch_rsa_pss_verify. launch_rsa_sign_selftest: an add's consistency run
// over the one row the host has put into the table's scratch.
size_t rsa_signtab_bytes();
hipError_t launch_rsa_sign_keyed(const uint32_t* stab, const uint32_t* key_id, const uint8_t* msgs,
                                 const uint64_t* msg_off, uint32_t msg_len, const uint8_t* salts, const uint8_t* gate,
                                 uint32_t W, uint64_t n, uint8_t* sigs, uint16_t* sig_len, uint8_t* status,
                                 uint8_t* ws, uint64_t ws_rows, hipStream_t s);
hipError_t launch_rsa_sign_selftest(uint32_t* stab, uint32_t W, hipStream_t s);
hipError_t launch_ecdsa_sign(const uint8_t* scheme, const uint8_t* seeds, const uint8_t* msgs, uint32_t msg_len,
                             uint64_t n, const uint32_t* gk1, const uint32_t* gr1, uint8_t* keys, uint8_t* key_len,
                             uint8_t* sigs, uint8_t* sig_len, hipStream_t s);
// K23 (sig_pack.hip, sig_pack.hpp): a mixed-scheme CSR batch in device memory classified
// and packed into the dense rows of the engines above -- count, scan and pack passes on
// s, nothing read back; the class counts stay in out.hdr. launch_sig_gather: a class's
// message rows (rows[r] = msgs[idx[r]], r below *count; cap: the host's upper bound).
// launch_sig_scatter: status[lane_of_row[r]] = row_status[r] for the same rows.
// launch_rsa_pss_verify_counted (rsa.hip): launch_rsa_pss_verify over dense messages and
// *count <= n rows; launch_count: rsa_counted_launches(n, ws_rows) words of scratch.
namespace sigpack {
struct In;
struct Out;
}  // namespace sigpack
hipError_t launch_sig_pack(const sigpack::In& in, const sigpack::Out& out, hipStream_t s);
hipError_t launch_sig_gather(const uint8_t* msgs, uint32_t msg_len, const uint32_t* idx, const uint32_t* count,
                             uint64_t cap, uint8_t* rows, hipStream_t s);
hipError_t launch_sig_scatter(const uint8_t* row_status, const uint32_t* lane_of_row, const uint32_t* count,
                              uint64_t cap, uint8_t* status, hipStream_t s);
// rows[s] = the transaction whose signature s is (tx_sig_off[ntx + 1]), s < nsig
hipError_t launch_sig_tx_rows(const uint64_t* tx_sig_off, uint64_t ntx, uint64_t nsig, uint32_t* rows, hipStream_t s);
uint64_t rsa_counted_launches(uint64_t n, uint64_t ws_rows);
hipError_t launch_rsa_pss_verify_counted(const uint32_t* mod, const uint32_t* exp, const uint8_t* sigs,
                                         const uint16_t* sig_len, const uint8_t* msgs, uint32_t msg_len, uint32_t W,
                                         uint64_t n, const unsigned int* count, const unsigned int* iota,
                                         unsigned int* launch_count, uint8_t* status, uint8_t* ws, uint64_t ws_rows,
                                         uint32_t flags, hipStream_t s);

namespace rt {

// The library's device memory per HIP device (every DevBuf, the fixed tables
// included): bytes in use and their peak, for cordahip_device_mem and the budget
// (CORDAHIP_DEVICE_MEM_BUDGET) that sizes the workspaces. Process-wide: every
// context (and test replica) on one GPU charges the same account.
constexpr int kMaxHipDevices = 32;  // cordahip_init takes a 32-bit device mask
struct MemAcct {
  std::atomic<uint64_t> in_use{0}, peak{0};
  void add(uint64_t b) {
    const uint64_t now = in_use.fetch_add(b) + b;
    uint64_t p = peak.load();
    while (now > p && !peak.compare_exchange_weak(p, now)) {
    }
  }
  void sub(uint64_t b) { in_use.fetch_sub(b); }
};
inline MemAcct& mem_acct(int dev) {
  static MemAcct acct[kMaxHipDevices];
  assert(dev >= 0 && dev < kMaxHipDevices);
  return acct[dev];
}

// grow-only device buffer, accounted on its owner's HIP device (Device::bind)
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int dev = -1;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) {
      cap = bytes;
      mem_acct(dev).add(bytes);
    } else {
      p = nullptr;
    }
    return e;
  }
  void release() {
    if (p) {
      (void)hipFree(p);
      mem_acct(dev).sub(cap);
    }
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// grow-only page-locked host buffer (staging for the packed host pipelines)
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes, unsigned flags = hipHostMallocDefault) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(&p, bytes, flags);
    if (e == hipSuccess) cap = bytes;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// The event that fences buffers shared between streams: every user makes its
// stream wait for the previous user's work, then records its own. Created on
// first use; a fence never recorded holds nobody back.
struct Fence {
  hipEvent_t ev = nullptr;
  hipError_t create() { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming); }
  hipError_t sync() const { return ev ? hipEventSynchronize(ev) : hipSuccess; }  // the host waits
  hipError_t wait(hipStream_t s) { return create() ? hipErrorUnknown : hipStreamWaitEvent(s, ev, 0); }
  hipError_t record(hipStream_t s) { return create() ? hipErrorUnknown : hipEventRecord(ev, s); }
  // Growing a buffer frees the smaller one, which the previous user's kernels (on
  // whatever stream) may still be using: the host waits for them first. `ensure`
  // ensures every buffer behind this fence; it runs only when `needed`.
  template <class G>
  hipError_t grow(bool needed, G&& ensure) const {
    if (!needed) return hipSuccess;
    const hipError_t e = sync();
    return e ? e : ensure();
  }
};
// The bracket of every launch that uses what the fences `fs` guard (the owner's lock
// held): s waits for each fence's previous user, then `launch` -- if the waits
// succeeded -- and each fence is recorded on s whatever the launch answered, so what
// was launched is fenced also after a failure. The first error.
template <class L>
hipError_t fenced(std::initializer_list<Fence*> fs, hipStream_t s, L&& launch) {
  hipError_t e = hipSuccess;
  for (Fence* f : fs) e = e ? e : f->wait(s);
  e = e ? e : launch();
  for (Fence* f : fs) {
    const hipError_t r = f->record(s);
    e = e ? e : r;
  }
  return e;
}

// What a struct below owns, it names once: its visit(v) passes every such member to
// one of these. A visitor derives from Visitor and redefines what it acts on; events,
// fences and streams may be null (created on first use).
enum : bool { kFreed = false, kKept = true };
struct Visitor {
  void dev(DevBuf&, bool /*keep: derived data the idle release leaves in place*/) {}
  void pin(PinBuf&, bool /*keep*/) {}
  void fence(Fence&) {}
  // staged: marks a pipeline stage's buffers free (the idle release waits for it, as for a fence)
  void event(hipEvent_t&, bool /*staged*/) {}
  void stream(hipStream_t&) {}
};

// one stage (buffer set) of the C5 streaming pipeline (cordahip_stream_verify);
// its events order the reuse of the buffers, so the host never waits per chunk
struct StreamStage {
  hipEvent_t ed_copied = nullptr, ec_copied = nullptr;  // this chunk's H2D of each section done
  hipEvent_t ed_done = nullptr, ec_done = nullptr;      // its kernels and status D2H done: buffers free
  DevBuf ed_keys, ed_sigs, ed_msgs, ed_status;
  DevBuf ec_scheme, ec_keys, ec_key_len, ec_sigs, ec_sig_len, ec_msgs, ec_status;
  template <class V>
  void visit(V& v) {
    for (hipEvent_t* e : {&ed_copied, &ec_copied, &ed_done, &ec_done}) v.event(*e, false);
    for (DevBuf* b : {&ed_keys, &ed_sigs, &ed_msgs, &ed_status, &ec_scheme, &ec_keys, &ec_key_len, &ec_sigs,
                      &ec_sig_len, &ec_msgs, &ec_status})
      v.dev(*b, kFreed);
  }
};
constexpr int kStreamStages = 3;
// lanes per chunk, both sections together (C5 A/B on one box, profiles/r02_c5_stream_ab.json:
// 2^21 76.7, 2^22 82.4, 2^23 84.9, 2^24 84.6 M verifs/s with the single-stream stages)
constexpr uint64_t kStreamChunk = 1ull << 23;

// one stage of a packed host pipeline (host_batch.cpp): the host packs a chunk
// of lanes into the pinned buffers, they cross PCIe into the device buffers,
// the kernels run, the statuses come back into h_status; `done` marks the
// stage reusable (the host scatters its statuses first)
struct PackStage {
  hipEvent_t copied = nullptr, done = nullptr;
  PinBuf h[9];
  DevBuf d[9];
  bool pending = false;
  uint64_t tag0 = 0, tag1 = 0, tag2 = 0;  // which chunk is in flight (pipeline-defined)
  template <class V>
  void visit(V& v) {
    for (hipEvent_t* e : {&copied, &done}) v.event(*e, false);
    for (PinBuf& b : h) v.pin(b, kFreed);
    for (DevBuf& b : d) v.dev(b, kFreed);
  }
};
constexpr int kPackStages = 3;
// Signed-tx batches keep more of their small (2^17-signature) chunks in flight:
// a chunk's prep waits for its id slice, and with three stages the pipeline could
// not run far enough ahead of the id chain -- c4h --components at two calls in
// flight 79.4-82.5 M sig/s with 3 stages, 84.7-85.7 with 4, 86.3-87.1 with 5,
// 86.4-87.6 with 6; c4h 90.3-91.5 / 90.6-91.5 / 89.3-92.6 / 92.4-92.5
// (profiles/r06_pack_stages_ab/). Generic batches (4 M-lane chunks, ~0.55 GB of
// pinned rows each) keep three.
#ifndef CORDAHIP_TX_STAGES
#define CORDAHIP_TX_STAGES 6  // A/B builds: -DCORDAHIP_TX_STAGES=N
#endif
constexpr int kTxStages = CORDAHIP_TX_STAGES;

// one stage of the generic-batch pipeline (host_batch.cpp): a chunk of the
// batch's lanes, classified and packed into BOTH sections' pinned buffers
// (h/d[0..4] Ed25519 keys, sigs, msgs, pre-status, status; [5..13] ECDSA
// scheme, keys, key_len, sigs, sig_len, msgs, msg_off, pre-status, status);
// the lane lists say where each row's status goes back.
// Signed-tx chunks with cordahip_set_rsa_on_device on carry a third section, the
// chunk's RSA_SHA256 lanes (rh/rd[0..5]: moduli, exponents, signatures, signature
// lengths, each row's id index, statuses; rd[6]: the gathered ids; the width classes'
// rows one class after the other); rsa_rows: its rows in flight (rsa_done follows them).
struct BatchStage {
  hipEvent_t copied = nullptr, ed_done = nullptr, ec_done = nullptr, rsa_done = nullptr;
  PinBuf h[14];
  DevBuf d[14];
  PinBuf hidx[2];  // device-id messages (MsgView::dev): per Ed25519 / ECDSA row, its tx's id index
  DevBuf didx[2];
  PinBuf rh[6];
  DevBuf rd[7];
  std::vector<uint64_t> ed_lanes, ec_lanes, rsa_lanes;
  uint64_t rsa_rows = 0;
  uint64_t a = 0, b = 0;  // the chunk's lanes [a, b) (per-chunk verdict words)
  bool direct = false;    // rows == lanes: statuses / verdict words went straight to the caller's pinned arrays
  DevBuf dverdict;        // the direct chunks' verdict words (wave ballots of the Ed25519 kernel)
  bool pending = false;
  template <class V>
  void visit(V& v) {
    for (hipEvent_t* e : {&copied, &ed_done, &ec_done, &rsa_done}) v.event(*e, true);
    for (PinBuf& b : h) v.pin(b, kFreed);
    for (DevBuf& b : d) v.dev(b, kFreed);
    for (PinBuf& b : hidx) v.pin(b, kFreed);
    for (DevBuf& b : didx) v.dev(b, kFreed);
    for (PinBuf& b : rh) v.pin(b, kFreed);
    for (DevBuf& b : rd) v.dev(b, kFreed);
    v.dev(dverdict, kFreed);
  }
};

struct TxWork {  // device buffers of the transaction paths (grow-only)
  DevBuf leaf_bytes, leaf_off, tx_leaf_off, hashes, txid, tx_status, tx_sig_off, msgs;
  DevBuf comp_items, payload, comp_status;  // component-level batches: items, their payload, encoder statuses
  DevBuf tok, tok_hash, tx_tok_off, root, stack;  // filtered-tx (partial Merkle tree) path
  DevBuf incl, tx_ntok, pmt_up, pmt_has;          // filtered-tx build: filter bytes, token counts, tree levels
  template <class V>
  void visit(V& v) {
    for (DevBuf* b : {&leaf_bytes, &leaf_off, &tx_leaf_off, &hashes, &txid, &tx_status, &tx_sig_off, &msgs,
                      &comp_items, &payload, &comp_status, &tok, &tok_hash, &tx_tok_off, &root, &stack, &incl,
                      &tx_ntok, &pmt_up, &pmt_has})
      v.dev(*b, kFreed);
  }
};

// One set of a device's transaction and signature-pipeline buffers. A call
// holds its set from start to finish; tx_ev marks the completion of the last
// work enqueued on the set's device buffers (the next holder's first wait).
struct TxSet {
  TxWork tx;
  Fence tx_ev;
  BatchStage pb[kTxStages];  // generic CSR batches (the first kPackStages) and the signed-tx signature chunks
  // component calls: the encoder's usage counters after this set's last call,
  // host-mapped: [templates in the arena, table slots in use, misses of set 0, of set 1]
  PinBuf kryo_usage;
  uint32_t* kryo_usage_dev = nullptr;
  // the device signed-tx calls' fork / join: the id chain runs on the id stream beside
  // the key half of the Ed25519 prep on the caller's stream
  hipEvent_t fork = nullptr, ids = nullptr;
  // their chunked Ed25519 section (ed_verify_device_chunks): s_ed2 forks off the
  // caller's stream and joins it again
  hipEvent_t ed_fork = nullptr, ed_join = nullptr;
  template <class V>
  void visit(V& v) {
    tx.visit(v);
    v.fence(tx_ev);
    for (BatchStage& st : pb) st.visit(v);
    v.pin(kryo_usage, kKept);
    for (hipEvent_t* e : {&fork, &ids, &ed_fork, &ed_join}) v.event(*e, false);
  }
};
constexpr int kTxSets = 2;

struct EcWork {  // device buffers of the ECDSA paths (grow-only)
  DevBuf counters, perm;
  DevBuf ws;  // split-kernel workspace (kEcWsSlots records)
  // the slot's routing scratch (K15, ecdsa_route.hpp: the gathered records and 4 bytes
  // per lane, grown in powers of two), behind the same lock and fence, released with
  // the workspace
  DevBuf route;
  Fence ev;  // last enqueued user of counters/perm/ws/route (cross-stream reuse)
  template <class V>
  void visit(V& v) {
    v.dev(counters, kKept);
    v.dev(perm, kFreed);
    v.dev(ws, kFreed);
    v.dev(route, kFreed);
    v.fence(ev);
  }
};

// RSA (rsa.hip): the verify launches' workspace and the single stage of the
// generic batches' RSA section (h/d[0..6]: moduli, exponents, signatures,
// signature lengths, messages, message offsets, statuses). Nothing here is
// allocated before a device's first RSA lane. route: the workspace's routing scratch
// (K20, rsa_route.hpp: a 64-byte header and 12 bytes per row of the largest launch),
// behind the same lock and fence, released with the workspace.
struct RsaWork {
  DevBuf ws;
  DevBuf route;
  Fence ev;  // last enqueued user of ws and route (cross-stream reuse)
  PinBuf h[7];
  DevBuf d[7];
  template <class V>
  void visit(V& v) {
    v.dev(ws, kFreed);
    v.dev(route, kFreed);
    v.fence(ev);
    for (PinBuf& b : h) v.pin(b, kFreed);
    for (DevBuf& b : d) v.dev(b, kFreed);
  }
};

// The mixed-scheme device calls' scratch (K23, cordahip_sig_verify_device): the counter
// block, the lanes' code bytes, the block totals and every class's packed rows, message
// rows and row statuses in `rows`; the RSA classes' in rsa_rows, which stays empty until
// a call asks for RSA on the device. Grow-only, behind Device::sigpack_mu and ev.
struct SigPackWork {
  DevBuf rows, rsa_rows;
  Fence ev;
  template <class V>
  void visit(V& v) {
    v.dev(rows, kFreed);
    v.dev(rsa_rows, kFreed);
    v.fence(ev);
  }
};

// The key table of one registered-key family on one device. It is allocated (zeroed) by
// the context's first add of the family, counted in the device's account like every
// DevBuf, and then kept until ~Device: the idle release and cordahip_trim never see it
// (Device::visit leaves it out; Device::visit_keys is for bind and ~Device), so nobody
// loses registered keys to an idle timer. ev: the fence of the kernels that read the
// table. stage: page-locked bytes a key goes out and its answer comes back in.
// A family derives from it and says how a slot of it is cleared (keyed.cpp clear_slot):
// record(slot), the bytes of tab to zero once ev has been waited for, and forget(slot),
// the host's note of the slot dropped. A signer family adds secrets(), the bytes
// cordahip_shutdown zeroes (signer_wipe). record() and secrets() are defined in
// keyed.cpp, where the kernels' layouts are known. A new family is such a struct and one
// line in Device::signer_keys or Device::verify_keys.
struct TabSpan {
  size_t at, bytes;
};
struct KeyTable {
  DevBuf tab;
  PinBuf stage;
  Fence ev;
  void forget(uint32_t) {}
  template <class V>
  void visit(V& v) {
    v.dev(tab, kKept);
    v.pin(stage, kKept);
    v.fence(ev);
  }
};

// What the host knows of a table of both ECDSA curves' keys, under the table's lock:
// built: the curve's table (the signer's comb, the verifier's base-point table) has been
// built; live: the curve's live keys on this device; of[slot]: the scheme of the slot's
// live record (0: none). Only curve() knows the index (0: secp256k1, 1: P-256).
template <uint32_t Slots>
struct CurveBook {
  uint32_t built[2] = {0, 0};
  uint32_t live[2] = {0, 0};
  uint8_t of[Slots] = {};
  static constexpr uint32_t curve(uint32_t scheme) { return scheme - 2; }
  bool table_built(uint32_t scheme) const { return built[curve(scheme)] != 0; }
  void mark_built(uint32_t scheme) { built[curve(scheme)] = 1; }
  void take(uint32_t slot, uint32_t scheme) {
    of[slot] = (uint8_t)scheme;
    live[curve(scheme)]++;
  }
  void drop(uint32_t slot) {
    if (of[slot]) live[curve(of[slot])]--;
    of[slot] = 0;
  }
  bool has_live(uint32_t scheme) const { return live[curve(scheme)] > 0; }
  bool any_live() const { return live[0] || live[1]; }
};

// The Ed25519 signer's (ed25519_comb.hpp: 4,096 records of 128 bytes and the expansion
// kernel's scratch): private keys, so cordahip_shutdown zeroes it before ~Device frees
// it. stage: 64 bytes, the seed out and the public key back (wiped before add returns).
struct SignKeys : KeyTable {
  TabSpan record(uint32_t slot) const;
  TabSpan secrets() const;
};

// The ECDSA signer's (ecdsa_sign_core.hpp: the two curves' comb tables, 4,096 records of
// 128 bytes and the add kernel's scratch): private keys, zeroed by cordahip_shutdown like
// SignKeys (the comb tables are public and stay). stage: 128 bytes, d out and the answer
// with Q back (d wiped before add returns). book: the curves' comb tables and live keys
// (CurveBook), under Device::sign_mu.
struct EcSignKeys : KeyTable {
  CurveBook<kSignKeySlots> book;
  TabSpan record(uint32_t slot) const;
  TabSpan secrets() const;
  void forget(uint32_t slot) { book.drop(slot); }
};

// The RSA signer's (rsa_sign.hpp: a slot -> record index over the pool's 4,096 slots, 64
// records of 3,360 bytes -- n, n', K, qR and the secret p, q, dP, dQ, qInv with their
// Montgomery constants -- and the scratch of an add's consistency run; 232,496 bytes):
// private keys, zeroed by cordahip_shutdown like SignKeys (the index stays). The host
// builds a record and it crosses in stage (wiped before add returns). rec_of / used:
// which record a slot's key took (index + 1; 0: none) and which records are taken,
// under Device::sign_mu.
struct RsaSignKeys : KeyTable {
  uint8_t rec_of[kSignKeySlots] = {};
  uint8_t used[64] = {};
  int take(uint32_t slot) {  // the first free record for the slot's key, or -1
    for (int r = 0; r < 64; r++)
      if (!used[r]) {
        used[r] = 1;
        rec_of[slot] = (uint8_t)(r + 1);
        return r;
      }
    return -1;
  }
  TabSpan record(uint32_t slot) const;
  TabSpan secrets() const;
  void forget(uint32_t slot) {
    if (rec_of[slot]) used[rec_of[slot] - 1] = 0;
    rec_of[slot] = 0;
  }
};

// The Ed25519 verification keys' (ed25519_vkey.hpp: 64 window tables of 512 KiB and the
// base point's, their records and the build kernel's scratch). stage: 64 bytes, the key
// bytes out and the decode verdict back. live: the slots whose record is live on this
// device (bit per slot, Device::vkey_mu): routed enqueues (K14) ask for it. route_tot:
// the device's cumulative counters of routed lanes (K14: keyed, generic; two 64-bit
// words, zeroed when allocated by the first routed enqueue), written by kernels ordered
// by ev. Clearing a slot leaves the window table: without a record whose id matches, no
// lane reads it.
struct RoutedKeyTable : KeyTable {
  DevBuf route_tot;
  template <class V>
  void visit(V& v) {
    KeyTable::visit(v);
    v.dev(route_tot, kKept);
  }
};
struct VerifyKeys : RoutedKeyTable {
  uint64_t live = 0;
  TabSpan record(uint32_t slot) const;
  void forget(uint32_t slot) { live &= ~(1ull << slot); }
};

// The ECDSA verification keys' (ecdsa_vkey.hpp: 64 window tables of 320 KiB, the two
// curves' base-point tables, the records and the build kernel's scratch). stage: 128
// bytes, the SEC1 bytes out and the decode verdict back. route_tot: as VerifyKeys' (K15).
// book: the curves' base-point tables and live keys (CurveBook), under Device::vkey_mu.
struct EcVerifyKeys : RoutedKeyTable {
  CurveBook<kVkeySlots> book;
  TabSpan record(uint32_t slot) const;
  void forget(uint32_t slot) { book.drop(slot); }
};

// The RSA verification keys' (rsa_vkey.hpp: 64 records of 1,056 bytes -- id, e, bit
// length, width class, n', n and K = R^e mod n -- 67,584 bytes). The host builds a
// record and it crosses in stage (1,056 bytes); no kernel builds anything. Allocated by
// a device's first RSA add, under Device::vkey_mu like the other families' tables.
// live: the slots whose record is live on this device (bit per slot, Device::vkey_mu):
// routed enqueues (K20) ask for it. route_tot: as VerifyKeys' (K20).
struct RsaVerifyKeys : RoutedKeyTable {
  uint64_t live = 0;
  TabSpan record(uint32_t slot) const;
  void forget(uint32_t slot) { live &= ~(1ull << slot); }
};

// a page-locked buffer and its twin on the device (ensure: true when it failed)
struct StageBuf {
  PinBuf h;
  DevBuf d;
  bool ensure(size_t bytes) { return h.ensure(bytes) != hipSuccess || d.ensure(bytes) != hipSuccess; }
  hipError_t to_device(size_t bytes, hipStream_t s) { return hipMemcpyAsync(d.p, h.p, bytes, hipMemcpyHostToDevice, s); }
  hipError_t to_host(size_t bytes, hipStream_t s) { return hipMemcpyAsync(h.p, d.p, bytes, hipMemcpyDeviceToHost, s); }
};
// The chunk stage of a registered-key host call (keyed.cpp keyed_chunks): page-locked
// buffers the host packs a chunk's lanes into and their twins on the device. Every call
// uses ids (key ids), msgs, msg_off and msg_len (the messages, with offsets and lengths
// when the chunk is not dense 32-byte rows) and status. cordahip_sign adds gate (gate
// bytes in) and sig_rows (64-byte signatures out); the verifiers add sig_rows (in: 64
// bytes a row, 72-byte DER slots for ECDSA), sig_len (ECDSA only), pre (the host's
// pre-statuses) and verdict (words out); cordahip_rsa_verify_keyed uses sig_rows (4 W-byte
// slots of one width class per launch), sig_len (uint16) and msg_off as a CSR of the
// launch's rows; cordahip_rsa_sign the same with sig_rows and sig_len (uint16) out, gate
// and salt (32 bytes a row) in. What a call does not use stays empty. mu is
// held for a shard's run; ev follows a chunk's last copy.
struct KeyedStage {
  std::mutex mu;
  StageBuf ids, msgs, msg_off, msg_len, status, gate, sig_rows, sig_len, pre, verdict, salt;
  Fence ev;
  template <class V>
  void visit(V& v) {
    for (StageBuf* b :
         {&ids, &msgs, &msg_off, &msg_len, &status, &gate, &sig_rows, &sig_len, &pre, &verdict, &salt}) {
      v.pin(b->h, kFreed);
      v.dev(b->d, kFreed);
    }
    v.fence(ev);
  }
};

// Fork-join pool for host-side packing and scattering. parallel_for splits
// [0, n) into pieces of at least `grain` lanes; the caller runs pieces too,
// so concurrent callers (one pipeline per device and section) all progress.
class HostPool {
 public:
  // cpus non-empty: every worker thread is bound to them (a device's NUMA node)
  explicit HostPool(int nthreads, const std::vector<int>& cpus = {});
  ~HostPool();
  int threads() const { return (int)threads_.size() + 1; }
  void parallel_for(uint64_t n, uint64_t grain, const std::function<void(uint64_t, uint64_t)>& fn);

 private:
  struct Job {
    const std::function<void(uint64_t, uint64_t)>* fn = nullptr;
    uint64_t n = 0, piece = 0, npieces = 0;
    std::atomic<uint64_t> next{0}, done{0};
    std::mutex m;
    std::condition_variable cv;
  };
  static void run_pieces(Job& j);
  void worker();
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<std::shared_ptr<Job>> q_;
  std::vector<std::thread> threads_;
  bool stop_ = false;
};

// Per-call timing of the *_device entry points: a ring of event pairs per
// device, one pair per call, so concurrent callers never share events; a
// slot's generation tells a reader whether its call's events are still there.
constexpr int kTimingRing = 64;
struct TimedCall {
  hipEvent_t a = nullptr, b = nullptr;
  uint64_t gen = 0;
};

struct Device {
  int id = 0;
  uint64_t uid = 0;  // process-unique: keys the per-thread timing slot
  // host threads next to this GPU (numa_place.hpp): the packing / scattering /
  // reduce pool of its pipelines, bound to CPUs of its NUMA node; the thread that
  // runs a pipeline binds itself there for the call (NodeBind), so the pinned
  // stages it allocates are first-touched on that node too
  NumaPlace place;
  std::unique_ptr<HostPool> pool;
  // device memory (CORDAHIP_DEVICE_MEM_BUDGET, cordahip_init): the workspace sizes
  // the budget allows -- Ed25519 slots 0 / 1 (lanes), ECDSA (slots) -- and the
  // activity the idle release reads (calls in progress, the last one's end)
  uint64_t mem_budget = 0;
  uint64_t ed_ws_lanes[2] = {0, 0};
  uint64_t ec_ws_slots = 0;
  std::atomic<int> active{0};
  std::atomic<int64_t> last_use_ms{0};
  DevBuf btab;              // the fixed-base tables, built once by cordahip_init
  DevBuf gtab_k1, gtab_r1;  // [k]G tables, k = 0..128, secp256k1 / P-256
  // ECDSA workspaces: slot 0 for the device path and the stream drain, slot 1 for the
  // host pipelines' alternate chunks (capped at half of slot 0), each with its lock;
  // ec_turn alternates the host chunks between them (s_ec / s_ec2)
  std::mutex ec_mu[2];
  EcWork ec[2];
  std::atomic<uint32_t> ec_turn{0};
  // RSA lanes: rsa_mu orders the users of the workspace (the dense device calls hold
  // it while they enqueue, a generic batch's RSA section for its whole run, stage
  // included); s_rsa is that section's stream, created with its first lane
  std::mutex rsa_mu;
  RsaWork rsa;
  // the mixed-scheme device calls (K23): sigpack_mu is held while such a call enqueues,
  // outside ed_mu[0], ec_mu[0] and rsa_mu, which it takes one after the other
  std::mutex sigpack_mu;
  SigPackWork sigpack;
  hipStream_t s_rsa = nullptr;
  hipStream_t stream = nullptr;  // context stream (init-time work and host tx paths)
  std::mutex tmu;
  TimedCall ring[kTimingRing];
  uint64_t ring_next = 0;
  // Transaction / signature-pipeline buffer sets (TxSet): a call holds one set
  // from start to finish (acquire_set / SetLease); two sets let a signed-tx call
  // drain while the next one enqueues. tx_order_mu is the enqueue token of the
  // signed-tx path: held from a call's start until its last chunk is enqueued,
  // so consecutive calls' work reaches the shared streams in call order.
  TxSet set[kTxSets];
  std::mutex set_m;
  std::condition_variable set_cv;
  bool set_busy[kTxSets] = {};
  std::mutex tx_order_mu;
  // consecutive Ed25519 chunks of every pipeline call alternate workspace slots and
  // streams (s_ed / s_ed2) across calls too, so call k + 1's first prep overlaps
  // call k's last ladder
  std::atomic<uint32_t> ed_turn{0};
  // Ed25519 split-kernel workspace, shared by every stream that verifies on
  // this device: ed_mu orders the enqueues, ed_ev makes each user's stream
  // wait for the previous user's kernels before it reuses the buffer.
  // Two workspace slots: the host pipelines alternate consecutive chunks between
  // them and between s_ed / s_ed2, so chunk k + 1's kernels fill the CUs chunk
  // k's end-of-grid tail leaves idle (slot 0 alone serves the device paths).
  // ed_route: the slot's routing scratch (K14, ed25519_route.hpp: 12 bytes per lane
  // and a header, grown in powers of two), behind the same lock and fence, released
  // with the workspace.
  std::mutex ed_mu[2];
  DevBuf ed_ws[2];
  DevBuf ed_route[2];
  Fence ed_ev[2];
  // The pipelines' three streams, created together and shared by the C5 drain
  // and the packed host pipelines: every H2D on s_copy (PCIe in chunk order),
  // each section's kernels + status D2H on its own stream. Three active
  // streams, not one per stage and section: HIP maps streams onto
  // GPU_MAX_HW_QUEUES (4) hardware queues, and streams sharing a queue
  // serialise (with 6 stage streams C5 ran 90.6 M/s at 4 queues, 93.4 at 8).
  std::mutex streams_mu;
  hipStream_t s_copy = nullptr, s_ed = nullptr, s_ec = nullptr, s_ed2 = nullptr;
  hipStream_t s_ec2 = nullptr;  // = s_idcopy: generic batches' alternate ECDSA chunks
  // signed-tx batches: the id slices' leaf-byte H2D on a stream of its own, so
  // slice j + 1's bytes cross PCIe while slice j hashes (d.stream)
  hipStream_t s_idcopy = nullptr;
  std::mutex stream_mu;  // serialises use of sstage (C5)
  StreamStage sstage[kStreamStages];
  // packed dense Ed25519 rows (cordahip_ed25519_verify_host); the generic CSR
  // batches' stages live in the TxSets
  std::mutex ped_mu;
  PackStage ped[kPackStages];
  // GPU Kryo encoder scratch (cordahip_kryo_encode_device): leaf sizes, the
  // scan's temporary storage, the shape table and templates, per-item shape
  // slots and the direct-encoder list, the direct writers' OutputChunked level
  // buffers; kryo_mu orders the enqueues, kryo_ev fences reuse
  std::mutex kryo_mu;
  DevBuf kryo_sizes, kryo_temp, kryo_ws, kryo_fixed, kryo_items;
  // the fixed part is persistent (shape table, records, templates): zeroed when
  // allocated, cleared when a call reports it over half full (TxSet::kryo_usage:
  // a host-mapped copy of its usage counters, stored after each call)
  bool kryo_fresh = false;
  bool kryo_templates_ok = false;  // the last component batch had no encoder misses (cordahip.cpp)
  PinBuf kryo_usage;               // cordahip_kryo_encode_device's own report
  uint32_t* kryo_usage_dev = nullptr;
  uint64_t kryo_gen = 0;           // table clears so far (kryo_mu): a call's end updates kryo_templates_ok
                                   // only if no clear came after its start
  Fence kryo_ev;
  // cordahip_tx_cover_device: the trees' evaluation stacks (8 B per token);
  // cover_mu orders the enqueues, cover_ev fences the scratch across streams
  std::mutex cover_mu;
  DevBuf cover_stack;
  Fence cover_ev;
  // Ed25519 signing (K11). The comb table [d 16^j]B sits in btab's allocation, after
  // the B tables (comb()), built with them by cordahip_init. keys: the key records
  // (SignKeys). sign_mu orders every user of the key table: a signing call holds it
  // while it enqueues -- its stream waits for keys.ev, its kernel is followed by
  // keys.ev whatever the launch answered (fenced) -- and add / remove hold it for their
  // whole run; remove waits for keys.ev first, so no kernel still reads the record it
  // zeroes.
  SignKeys keys;
  // ECDSA signing (K17): the records of the same registry's ECDSA keys and the curves'
  // comb tables, an allocation of their own under the same sign_mu, with a fence of
  // their own (ec_keys.ev) that add, remove and every signing call use as keys.ev is used.
  EcSignKeys ec_keys;
  // RSA signing (K19): the records of the same registry's RSA keys, an allocation of
  // their own under the same sign_mu, with a fence of their own. The signing calls borrow
  // the RSA workspace, so they take rsa_mu first, as every user of it does, and sign_mu
  // inside it: the host call rsa_mu -> sign_stage.mu -> sign_mu (per launch), the device
  // call rsa_mu -> sign_mu. The workspace grows before sign_mu is taken.
  RsaSignKeys rsa_keys;
  std::mutex sign_mu;
  uint32_t* comb() const { return reinterpret_cast<uint32_t*>(static_cast<char*>(btab.p) + ed25519_btable_bytes()); }
  // the chunk stage of cordahip_sign and cordahip_ecdsa_sign (KeyedStage)
  KeyedStage sign_stage;

  // Ed25519 verification against registered keys (K12). vkeys: the key tables
  // (VerifyKeys). vkey_mu orders every user of them exactly as sign_mu orders the
  // signer's: a keyed verification holds it while it enqueues -- its stream waits for
  // vkeys.ev, its kernel is followed by vkeys.ev -- and add / remove hold it for their
  // whole run; remove waits for vkeys.ev first.
  // Routing (K14, cordahip_vkey_set_routing): with route_on set and a live Ed25519
  // key (vkeys.live), ed_verify_enqueue is a keyed call too: under ed_mu[slot] it takes
  // vkey_mu for the route pass and the K12 launch -- behind vkeys.ev, followed by
  // vkeys.ev -- and drops it before the generic engine. With route_on clear it takes no
  // lock it did not take before.
  // Lock order of the locks met on these paths, outermost first:
  //   ped_mu / stream_mu / a SetLease (the pipelines) -> sigpack_mu -> ed_mu[0] -> ed_mu[1] ->
  //   ec_mu[0] -> ec_mu[1] -> rsa_mu -> ... -> sign_stage.mu -> vkey_stage.mu -> vkey_mu.
  // sign_mu stands where vkey_mu does, inside sign_stage.mu; no path holds both.
  // trim_device takes them in that order up to vkey_stage.mu; a keyed host call holds
  // its stage's mu for a shard's run (keyed.cpp ShardRun) and takes sign_mu / vkey_mu
  // inside it, around an enqueue only; a routed enqueue holds ed_mu[slot] (Ed25519, K14)
  // or ec_mu[slot] (ECDSA, K15) and takes vkey_mu inside it. vkey_mu is innermost:
  // whoever holds it (add, remove, the stats call, a keyed or routed enqueue) takes no
  // other lock of the device but tmu
  // (the timing ring's, a leaf held for a few assignments), and a routed enqueue never
  // holds it while it waits for another lock, the slot's fence or the scratch's growth.
  // The keyed RSA calls (K18) borrow the RSA workspace, so they take rsa_mu first, as
  // every user of it does, and vkey_mu inside it: the host call rsa_mu -> vkey_stage.mu
  // -> vkey_mu (per launch), the device calls rsa_mu -> vkey_mu (the raw op, which needs
  // no workspace, vkey_mu alone). The workspace grows before vkey_mu is taken.
  VerifyKeys vkeys;
  std::mutex vkey_mu;
  std::atomic<uint32_t> route_on{0};
  // ECDSA verification against registered keys (K13): the tables of the same registry's
  // ECDSA keys, under the same vkey_mu, with a fence of their own.
  // Routing (K15, cordahip_vkey_set_routing_ecdsa): with ec_route_on set and a live
  // ECDSA key (ec_vkeys.book), ec_verify_enqueue is a keyed call too: under the
  // caller's ec_mu[slot] it takes vkey_mu for the route pass and the K13 launches --
  // behind ec_vkeys.ev, followed by ec_vkeys.ev -- and drops it before the generic
  // engine. With ec_route_on clear it takes no lock it did not take before.
  EcVerifyKeys ec_vkeys;
  std::atomic<uint32_t> ec_route_on{0};
  // RSA verification against registered keys (K18): the records of the same registry's
  // RSA keys, under the same vkey_mu, with a fence of their own.
  // Routing (K20, cordahip_vkey_set_routing_rsa): with rsa_route_on set and a live RSA
  // key (rsa_vkeys.live), every launch of rsa_verify_enqueue is a keyed call too: under the
  // caller's rsa_mu it takes vkey_mu for the route pass and K18's exponentiation -- behind
  // rsa_vkeys.ev, followed by rsa_vkeys.ev -- and drops it before the generic
  // exponentiation and the check. With rsa_route_on clear it takes no lock it did not
  // take before.
  RsaVerifyKeys rsa_vkeys;
  std::atomic<uint32_t> rsa_route_on{0};
  // Routing inside the mixed device calls (K24, cordahip_vkey_set_routing_device): with
  // sig_route_on set, each family's section of sig_device_enqueue follows that family's
  // switch above and its live keys, with the family's scratch behind the family's lock
  // and fence: sigpack_mu -> the family's mutex -> vkey_mu, as the dense calls. Clear,
  // the mixed calls launch, allocate and lock what they did before K24.
  std::atomic<uint32_t> sig_route_on{0};
  // the chunk stage of cordahip_verify_keyed, cordahip_ecdsa_verify_keyed and
  // cordahip_rsa_verify_keyed (KeyedStage)
  KeyedStage vkey_stage;

  // everything but the key tables (signer_keys, verify_keys: visit_keys), which the idle
  // release is never offered
  template <class V>
  void visit(V& v) {
    for (DevBuf* b : {&btab, &gtab_k1, &gtab_r1}) v.dev(*b, kKept);
    vkey_stage.visit(v);
    sign_stage.visit(v);
    for (EcWork& w : ec) w.visit(v);
    rsa.visit(v);
    sigpack.visit(v);
    for (hipStream_t* s : {&s_rsa, &stream, &s_copy, &s_ed, &s_ec, &s_ed2, &s_idcopy}) v.stream(*s);  // s_ec2 is s_idcopy
    for (TimedCall& tc : ring)
      for (hipEvent_t* e : {&tc.a, &tc.b}) v.event(*e, false);
    for (TxSet& S : set) S.visit(v);
    for (DevBuf& b : ed_ws) v.dev(b, kFreed);
    for (DevBuf& b : ed_route) v.dev(b, kFreed);
    for (Fence& f : ed_ev) v.fence(f);
    for (StreamStage& st : sstage) st.visit(v);
    for (PackStage& st : ped) st.visit(v);
    for (DevBuf* b : {&kryo_sizes, &kryo_temp, &kryo_ws, &kryo_items}) v.dev(*b, kFreed);
    v.dev(kryo_fixed, kKept);
    v.pin(kryo_usage, kKept);
    v.fence(kryo_ev);
    v.dev(cover_stack, kFreed);
    v.fence(cover_ev);
  }
  // before any allocation: the HIP device whose account the buffers charge
  void bind(int hip_id) {
    struct Bind : Visitor {
      int id;
      void dev(DevBuf& b, bool) { b.dev = id; }
    } v;
    id = v.id = hip_id;
    visit(v);
    visit_keys(v);
  }
  // The registered-key families as two walks, f(table) for each: the signer's registry's
  // (sign_mu) and the verification keys' (vkey_mu). A remove clears its slot in every
  // family of its walk (keyed.cpp clear_slot); cordahip_shutdown wipes the signer's.
  template <class F>
  void signer_keys(F&& f) {
    f(keys);
    f(ec_keys);
    f(rsa_keys);
  }
  template <class F>
  void verify_keys(F&& f) {
    f(vkeys);
    f(ec_vkeys);
    f(rsa_vkeys);
  }
  // every key table: bound and destroyed with the rest, never released while the
  // context lives
  template <class V>
  void visit_keys(V& v) {
    const auto visit_one = [&](auto& k) { k.visit(v); };
    signer_keys(visit_one);
    verify_keys(visit_one);
  }
  struct Release : Visitor {  // the buffers; all: the kept ones too
    bool all = false;
    void dev(DevBuf& b, bool keep) {
      if (all || !keep) b.release();
    }
    void pin(PinBuf& b, bool keep) {
      if (all || !keep) b.release();
    }
  };
  // the idle release's part once the caller holds every lock that guards a buffer
  // (trim_device): waits for the fences and the stages' events, then frees what is not kept
  void release_idle() {
    struct Quiesce : Visitor {
      void fence(Fence& f) { (void)f.sync(); }
      void event(hipEvent_t& e, bool staged) {
        if (staged && e) (void)hipEventSynchronize(e);
      }
    } q;
    visit(q);
    Release r;
    visit(r);
  }
  ~Device() {  // everything visited
    (void)hipSetDevice(id);
    struct Destroy : Release {
      void fence(Fence& f) { event(f.ev, false); }
      void event(hipEvent_t& e, bool) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
      }
      void stream(hipStream_t& s) {
        if (s) (void)hipStreamDestroy(s);
        s = nullptr;
      }
    } v;
    v.all = true;
    visit(v);
    visit_keys(v);
  }
};

// One notary commit log (K16, cordahip_commit_log_*): the table of consumed StateRefs
// on one device. Owned by the context's registry, not by the Device: cordahip_trim and
// the idle release never see it; destroy and cordahip_shutdown free it. Its buffers are
// counted in the device's account like every DevBuf. mu is held by every call on the
// log while it enqueues (and by destroy / reserve / stats / load for their whole run);
// ev follows each call's last kernel, and the next call's stream waits for it. bound:
// the host's upper bound of the live entries; next_seq: the sequence number of the
// next call's first transaction (loaded rows carry 0). counters: two 64-bit words on
// the device (live entries; the last load's rows already present). scratch and the
// stages grow only; stage_ev follows a host call's last copy. Ticketed commits take a
// turn number at submit and run in that order (turn_mu / turn_cv).
struct CommitLog {
  uint32_t id = 0;
  Device* dev = nullptr;
  std::mutex mu;
  DevBuf tab, counters, scratch, stage_d;
  PinBuf stage_h;
  Fence ev, stage_ev;
  uint32_t capacity_log2 = 0;
  uint64_t k0 = 0, k1 = 0;
  uint64_t bound = 0;
  uint64_t next_seq = 1;
  std::mutex turn_mu;
  std::condition_variable turn_cv;
  uint64_t turn_next = 0, turn_now = 0;
  commit::Table table() const { return commit::Table{tab.as<uint32_t>(), (1ull << capacity_log2) - 1, k0, k1}; }
  ~CommitLog() {
    if (dev) (void)hipSetDevice(dev->id);
    (void)ev.sync();
    (void)stage_ev.sync();
    for (DevBuf* b : {&tab, &counters, &scratch, &stage_d}) b->release();
    stage_h.release();
    for (Fence* f : {&ev, &stage_ev})
      if (f->ev) (void)hipEventDestroy(f->ev);
  }
};

// The calling thread bound to a device's CPUs for a scope (its previous affinity
// restored after): pipelines pack rows and first-touch pinned stages on the GPU's
// NUMA node. No-op when the device has no placement.
class NodeBind {
 public:
  explicit NodeBind(const Device& d);
  ~NodeBind();
  NodeBind(const NodeBind&) = delete;
  NodeBind& operator=(const NodeBind&) = delete;

 private:
  bool bound_ = false;
  std::vector<unsigned char> saved_;  // cpu_set_t bytes
};
// the pool a device's host work runs on
HostPool& pool_of(cordahip_ctx* ctx, Device& d);


// ---- ticket pool -------------------------------------------------------------
struct JobState {
  std::mutex m;
  std::condition_variable cv;
  bool done = false;
  int rc = CORDAHIP_SUCCESS;
};

class WorkerPool {
 public:
  explicit WorkerPool(int nthreads);
  ~WorkerPool();
  void push(std::shared_ptr<JobState> st, std::function<int()> fn);

 private:
  void run();
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<std::pair<std::shared_ptr<JobState>, std::function<int()>>> q_;
  std::vector<std::thread> threads_;
  bool stop_ = false;
};

// CORDAHIP_TRACE=1: host-side phase timings of the host pipelines on stderr
// (wait for a stage, classify, pack, enqueue; tx-id / signature phases), to
// see whether the host or the GPU bounds a host batch
inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline bool tracing() {
  static const bool on = getenv("CORDAHIP_TRACE") != nullptr;
  return on;
}

// a call in progress on a device (the idle release waits for none)
class Activity {
 public:
  explicit Activity(Device& d) : d_(d) { d_.active.fetch_add(1); }
  ~Activity() {
    d_.last_use_ms.store((int64_t)now_ms());
    d_.active.fetch_sub(1);
  }
  Activity(const Activity&) = delete;
  Activity& operator=(const Activity&) = delete;

 private:
  Device& d_;
};

// The device address of pinned host memory p (nullptr when p is pageable or
// unknown to HIP): kernels store results there directly, since a D2H
// hipMemcpyAsync queued behind busy compute streams can hold the enqueuing
// thread for milliseconds (7-9 ms per call in profiles/r04_q)
inline void* host_mapped(const void* p) {
  hipPointerAttribute_t at;
  void* dp = nullptr;
  if (!p || hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeHost ||
      hipHostGetDevicePointer(&dp, const_cast<void*>(p), 0) != hipSuccess)
    dp = nullptr;
  (void)hipGetLastError();
  return dp;
}

// under CORDAHIP_TRACE: report a HIP call that held the host for over 1 ms
template <class F>
hipError_t blocked(const char* what, F&& f) {
  if (!tracing()) return f();
  const double t = now_ms();
  const hipError_t e = f();
  const double dt = now_ms() - t;
  if (dt > 1.0) fprintf(stderr, "[cordahip] %s held the host %.2f ms\n", what, dt);
  return e;
}

int hip_err(hipError_t e);
// Entry points run host code that allocates (staging vectors, worker threads): no
// C++ exception may cross the C ABI into the JVM.
template <class F>
int guarded(F&& f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return CORDAHIP_ERR_OUT_OF_MEMORY;
  } catch (...) {
    return CORDAHIP_ERR_HIP;
  }
}
hipError_t ensure_streams(Device& d);
void trim_device(Device& d);  // the idle release of one device (cordahip_trim, the reaper)
// the Ed25519 section of a device signed-tx call, in chunks on two streams
hipError_t ed_verify_device_chunks(Device& d, TxSet& S, const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs,
                                   uint64_t n, uint8_t* status, hipStream_t s);
// before_msgs != nullptr: the messages are produced on stream s by that callback,
// which runs after the keys' half of the prep is enqueued (launch_ed25519_verify)
hipError_t ed_verify_enqueue(Device& d, const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs,
                             uint32_t msg_len, uint64_t n, const uint8_t* pre, uint8_t* status,
                             unsigned long long* verdict, uint32_t flags, hipStream_t s, int slot = 0,
                             const std::function<hipError_t()>* before_msgs = nullptr);
// d.ec_mu[slot] must be held
hipError_t ec_verify_enqueue(Device& d, const uint8_t* scheme, const uint8_t* keys, const uint8_t* key_len,
                             const uint8_t* sigs, const uint8_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off,
                             uint32_t msg_len, uint64_t n, const uint8_t* pre, uint8_t* status,
                             unsigned long long* verdict, uint32_t flags, hipStream_t s, int slot = 0);
// d.rsa_mu must be held: the RSA workspace grown for n rows of class W (at most the
// workspace's row cap; the launches loop over it), after its previous user's kernels
hipError_t rsa_ws_grow(Device& d, uint32_t W, uint64_t n);
// d.rsa_mu must be held; one width class per call (rsa.hip launch_rsa_pss_verify)
hipError_t rsa_verify_enqueue(Device& d, const uint32_t* mod, const uint32_t* exp, const uint8_t* sigs,
                              const uint16_t* sig_len, const uint8_t* msgs, const uint64_t* msg_off, uint32_t msg_len,
                              uint32_t W, uint64_t n, const uint8_t* pre, uint8_t* status,
                              unsigned long long* verdict, uint32_t flags, hipStream_t s);
// K23: a mixed-scheme batch in device memory (in: device pointers; msgs: in.msg_rows dense
// rows of in.msg_len bytes) packed and verified on s by the generic engines, whatever the
// routing switches say: statuses in lane order, verdict words when verdict is non-null.
// Takes sigpack_mu and, inside it, ed_mu[0], ec_mu[0] and rsa_mu in turn.
hipError_t sig_device_enqueue(Device& d, const sigpack::In& in, const uint8_t* msgs, uint8_t* status,
                              unsigned long long* verdict, hipStream_t s);
void shard_range(uint64_t n, uint64_t nshards, uint64_t shard, uint64_t align, uint64_t& lo, uint64_t& hi);
uint64_t env_lanes(const char* name, uint64_t dflt);

// Run fn(device, lo, hi) for every non-empty shard of n lanes, one host thread
// per device; returns the first failure.
template <class F>
int for_shards(std::vector<std::unique_ptr<Device>>& devs, uint64_t n, uint64_t align, F fn) {
  const uint64_t nd = devs.size();
  std::vector<std::future<int>> fs;
  for (uint64_t i = 0; i < nd; i++) {
    uint64_t lo, hi;
    shard_range(n, nd, i, align, lo, hi);
    if (lo >= hi) break;
    Device* d = devs[i].get();
    if (nd == 1) return fn(*d, lo, hi);
    fs.push_back(std::async(std::launch::async, [=, &fn] { return fn(*d, lo, hi); }));
  }
  int rc = CORDAHIP_SUCCESS;
  for (auto& f : fs) {
    const int r = f.get();
    if (r != CORDAHIP_SUCCESS && rc == CORDAHIP_SUCCESS) rc = r;
  }
  return rc;
}

// A device's buffer set for one call: the first free one (blocks while both are
// held); `prefer` is tried first. The holder then waits on set.tx_ev before
// touching device buffers an asynchronous device-path call may still use.
class SetLease {
 public:
  // exact: set `prefer` itself (the idle release takes both)
  explicit SetLease(Device& d, int prefer = 0, bool exact = false) : d_(d) {
    std::unique_lock<std::mutex> g(d.set_m);
    for (;;) {
      for (int k = 0; k < (exact ? 1 : kTxSets); k++) {
        const int i = (prefer + k) % kTxSets;
        if (!d.set_busy[i]) {
          d.set_busy[i] = true;
          idx_ = i;
          return;
        }
      }
      d.set_cv.wait(g);
    }
  }
  ~SetLease() {
    {
      std::lock_guard<std::mutex> g(d_.set_m);
      d_.set_busy[idx_] = false;
    }
    d_.set_cv.notify_one();
  }
  SetLease(const SetLease&) = delete;
  SetLease& operator=(const SetLease&) = delete;
  int index() const { return idx_; }
  TxSet& get() const { return d_.set[idx_]; }

 private:
  Device& d_;
  int idx_ = 0;
};

}  // namespace rt
}  // namespace cordahip

struct cordahip_ctx {
  std::vector<std::unique_ptr<cordahip::rt::Device>> devs;
  std::mutex mu;  // guards next_ticket and jobs
  uint64_t next_ticket = 1;
  std::unordered_map<uint64_t, std::shared_ptr<cordahip::rt::JobState>> jobs;
  std::unique_ptr<cordahip::rt::WorkerPool> pool;
  std::unique_ptr<cordahip::rt::HostPool> host;  // packing / scattering threads
  // signed-tx batches' signature -> transaction maps, kept for reuse across
  // calls (a fresh 20 MB map per C4 call page-faulted for 0.8-3.9 ms): taken
  // by a call, returned after it; at most kTxOfCache kept
  static constexpr size_t kTxOfCache = 4;
  std::mutex txof_mu;
  std::vector<std::pair<std::unique_ptr<uint64_t[]>, uint64_t>> txof_free;
  // the idle release (CORDAHIP_IDLE_RELEASE_MS): a thread that frees an idle
  // device's grow-only buffers (runtime.cpp trim_device)
  // the two key registries (key_slots.hpp): which slots are live and each slot's reuse
  // counter; no key material. Their ids are namespaces of their own.
  cordahip::rt::SignerSlots signers;  // cordahip_signer_add_ed25519 / _remove
  cordahip::rt::VkeySlots vkeys;      // cordahip_vkey_add_ed25519 / _add_ecdsa / _add_rsa / _remove
  // what the host knows of each slot's live RSA key (words 0: the slot holds none): the
  // keyed RSA host call sizes and partitions its rows from it without a device read
  struct RsaVkeyMirror {
    uint32_t id = 0, words = 0, bits = 0;
  };
  std::mutex rsa_mirror_mu;
  RsaVkeyMirror rsa_mirror[cordahip::kVkeySlots];
  // the same of the signer's live RSA keys (id, class and bits only: no key material),
  // under rsa_mirror_mu; rsa_signers: how many (at most CORDAHIP_RSA_SIGNER_MAX_KEYS),
  // under signers.mu
  RsaVkeyMirror rsa_sign_mirror[cordahip::kSignKeySlots];
  uint32_t rsa_signers = 0;
  // cordahip_set_rsa_on_device: the signed-tx host calls, whose structs carry no flags,
  // verify their RSA_SHA256 lanes on the GPU (CORDAHIP_FLAG_RSA_ON_DEVICE's counterpart)
  std::atomic<uint32_t> rsa_on_device{0};
  // the notary commit logs (cordahip_commit_log_create / _destroy): id -> log; ids
  // count up and are never reused. logs_mu guards the map and the counter only.
  std::mutex logs_mu;
  std::unordered_map<uint32_t, std::shared_ptr<cordahip::rt::CommitLog>> logs;
  uint32_t next_log_id = 1;
  std::thread reaper;
  std::mutex reaper_mu;
  std::condition_variable reaper_cv;
  bool reaper_stop = false;
};

namespace cordahip {
namespace rt {
// The ids of one device's transaction shard as its id slices leave them in HBM
// (signed-tx batches): txid[t - t0] is transaction t's id once the event of the
// slice holding t has completed; the signatures are verified in chunks whose
// message rows the device gathers from there (no host round trip for the ids).
struct DeviceIds {
  const uint8_t* txid = nullptr;           // device pointer, the shard's ids
  uint64_t t0 = 0;                         // the shard's first transaction
  std::vector<uint64_t> tx_bound;          // slice j = transactions [tx_bound[j], tx_bound[j + 1])
  std::vector<hipEvent_t> ready;           // ready[j]: slice j's ids are in txid (recorded on the id stream)
  std::vector<uint64_t> chunk_bound;       // the signature pipeline's chunk boundaries (signature indices)
  // Ed25519 chunks run the prep's key half before waiting for their ids (leaf
  // batches: +1.5% c4h interleaved; component batches, whose heavier id kernels
  // then meet more prep beside them: -1.8%, profiles/r05_prep_split_ab/)
  bool split_prep = false;
  // called before a chunk's copies are enqueued (after = false: the id slices
  // the chunk ending at sig_end needs) and after them (after = true: a few more)
  std::function<hipError_t(uint64_t sig_end, bool after)> advance;
  // called when the statuses of signatures [a, b) are final on the host (a
  // chunk has finished): the per-transaction reduce of the transactions whose
  // signatures all lie in [a, b) runs there, while later chunks verify
  std::function<hipError_t(uint64_t a, uint64_t b)> done;
  // called once every chunk is enqueued, before the pipeline drains: the signed-tx
  // call enqueues its remaining id slices and hands the enqueue token to the next call
  std::function<hipError_t()> enqueued;
  hipEvent_t wait_for(uint64_t tx) const {  // the event after which transaction tx's id is on the device
    const size_t j = (size_t)(std::upper_bound(tx_bound.begin(), tx_bound.end(), tx) - tx_bound.begin());
    return ready[j ? j - 1 : 0];
  }
};

// Where lane i's message is: the batch's CSR (msg + msg_off), or -- for the
// signatures of a transaction batch, each over its transaction's id
// (SignedTransaction.kt:98) -- the 32-byte id of transaction tx_of[i]: on the
// host at base (dev == nullptr) or on the device (dev).
struct MsgView {
  const uint8_t* base;
  const uint64_t* off;
  const uint64_t* tx_of;
  const DeviceIds* dev = nullptr;
  uint64_t chunk = 0;  // lanes per pipeline chunk (0: the default, CORDAHIP_HOST_CHUNK)
  const uint8_t* ptr(uint64_t i) const { return tx_of ? base + 32 * tx_of[i] : base + off[i]; }
  uint64_t len(uint64_t i) const { return tx_of ? 32 : off[i + 1] - off[i]; }
};
// generic CSR batches (host_batch.cpp); sig_verify_msgs takes the messages
// from mv instead of b->msg / b->msg_off
int sig_verify_impl(cordahip_ctx* ctx, const cordahip_sig_batch* b);
int sig_verify_msgs(cordahip_ctx* ctx, const cordahip_sig_batch* b, const MsgView& mv);
// lanes [lo, hi) of b on device d only, through the stages of the caller's set
// (the signed-tx path's per-device signatures)
int sig_verify_range(cordahip_ctx* ctx, Device& d, TxSet& set, const cordahip_sig_batch* b, const MsgView& mv,
                     uint64_t lo, uint64_t hi);
// dense Ed25519 rows in host memory through the packed pipeline (host_batch.cpp)
int ed25519_dense_host(cordahip_ctx* ctx, const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs,
                       uint32_t msg_len, uint64_t n, uint8_t* status, uint64_t* verdict);
void verdict_from_status(cordahip_ctx* ctx, const uint8_t* status, uint64_t n, uint64_t* verdict);
// every key record of every device zeroed (cordahip_shutdown, before the tables are freed)
void signer_wipe(cordahip_ctx* ctx);
// zero n bytes with a write the compiler cannot drop
void secure_wipe(void* p, size_t n);
}  // namespace rt
}  // namespace cordahip
