/* cordahip.h — C-ABI of libcordahip.so, the MI355X batch signature and
 * transaction-id verification engine for Corda's hot path.
 *
 * Drop-in boundary. Every entry point is plain C: pointers,
 * sizes, status codes; no C++ types or exceptions cross it, so a JNI shim (see
 * INTEGRATION.md) or ctypes binds it directly. The entry points replace:
 *
 *   cordahip_sig_submit / cordahip_sig_verify
 *       -> Crypto.isValid(scheme, key, sig, clear)   core/src/main/kotlin/net/corda/core/crypto/Crypto.kt:534-541
 *          Crypto.doVerify(scheme, key, sig, clear)  Crypto.kt:472-483
 *          (one call per signature today, through the JCA SPI at Crypto.kt:537-540;
 *           here: one call per BATCH, per-lane status instead of throw/false)
 *   cordahip_ed25519_verify_device / _host
 *       -> the EDDSA_ED25519_SHA512 lane of the above (Crypto.kt:119-132), dense layout
 *   cordahip_ed25519_sign_device
 *       -> Crypto.doSign(EDDSA_ED25519_SHA512, ...) (Crypto.kt:380-400) and
 *          deriveKeyPairFromEntropy (Crypto.kt:733-739): corpus generation only
 *   cordahip_tx_ids (tx id = Merkle root of component hashes)
 *       -> WireTransaction.id (WireTransaction.kt:48) = MerkleTree.getMerkleTree(
 *          availableComponentHashes).hash (MerkleTree.kt:27-66, MerkleTransaction.kt:69)
 *   cordahip_signed_tx_verify / cordahip_tx_submit
 *       -> SignedTransaction.checkSignaturesAreValid (SignedTransaction.kt:95-100)
 *          + the tx.id recomputation of verifySignatures (:70-85); signer coverage
 *          (getMissingSignatures :102-108) is the _covered forms below.
 *          The _submit forms return a ticket at once: the caller (a Quasar fiber in
 *          ResolveTransactionsFlow.call, ResolveTransactionsFlow.kt:97-122, on the
 *          single Node thread) suspends on it instead of blocking the thread.
 *   cordahip_*_covered / cordahip_tx_cover_device / cordahip_cover_eval_host
 *       -> SignedTransaction.getMissingSignatures (SignedTransaction.kt:102-108),
 *          CompositeKey.isFulfilledBy (CompositeKey.kt:186-209) and the
 *          SignaturesMissingException decision of verifySignatures (:76-82)
 *
 * Result contract: a return value < 0 means the whole call failed (the caller
 * falls back to the JVM path for that batch); per-lane outcomes are DATA in
 * status[] (CORDAHIP_STATUS_*), never return codes.
 *
 * Ownership: the caller owns every host buffer and must leave it untouched
 * until cordahip_wait()/poll() reports the ticket done. Buffers from
 * cordahip_alloc_pinned() are page-locked (hipHostMalloc) and are the fast
 * path for host batches. The library owns device memory and HIP streams.
 * A context is thread-safe: submit/wait/poll from any thread.
 */
#ifndef CORDAHIP_H
#define CORDAHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CORDAHIP_ABI_VERSION 4u

/* ---- per-lane statuses (status[i]) ------------------------------------- */
#define CORDAHIP_STATUS_OK 0            /* isValid -> true;  doVerify -> true                         */
#define CORDAHIP_STATUS_BAD_SIG 1       /* isValid -> false; doVerify -> SignatureException            */
#define CORDAHIP_STATUS_MALFORMED_SIG 2 /* SignatureException from the engine (bad length / DER)       */
#define CORDAHIP_STATUS_BAD_KEY 3       /* key decode failed (IllegalArgumentException at key build)   */
#define CORDAHIP_STATUS_UNSUPPORTED 4   /* IllegalArgumentException: unsupported scheme (Crypto.kt:474)*/
#define CORDAHIP_STATUS_EMPTY 5         /* IllegalArgumentException: empty sig / clear (Crypto.kt:475) */

/* ---- return codes -------------------------------------------------------- */
#define CORDAHIP_SUCCESS 0
#define CORDAHIP_ERR_INVALID_ARG (-1)
#define CORDAHIP_ERR_HIP (-2)
#define CORDAHIP_ERR_NO_DEVICE (-3)
#define CORDAHIP_ERR_OUT_OF_MEMORY (-4)
#define CORDAHIP_ERR_TIMEOUT (-5)
#define CORDAHIP_ERR_UNKNOWN_TICKET (-6)
#define CORDAHIP_ERR_NOT_IMPLEMENTED (-7)
/* -8 CORDAHIP_ERR_BUFFER_TOO_SMALL: see cordahip_kryo_encode */

/* ---- signature schemes = Corda SignatureScheme.schemeNumberID ------------ */
#define CORDAHIP_SCHEME_RSA_SHA256 1             /* Crypto.kt:77  (UNSUPPORTED lane unless CORDAHIP_FLAG_RSA_ON_DEVICE) */
#define CORDAHIP_SCHEME_ECDSA_SECP256K1_SHA256 2 /* Crypto.kt:92  */
#define CORDAHIP_SCHEME_ECDSA_SECP256R1_SHA256 3 /* Crypto.kt:106 */
#define CORDAHIP_SCHEME_EDDSA_ED25519_SHA512 4   /* Crypto.kt:120 */
#define CORDAHIP_SCHEME_SPHINCS256_SHA256 5      /* Crypto.kt:140 (not on GPU -> UNSUPPORTED lane) */

typedef struct cordahip_ctx cordahip_ctx;

uint32_t cordahip_abi_version(void);
const char* cordahip_strerror(int code);

/* device_mask: bit d selects visible HIP device d; 0 = all visible devices. */
int cordahip_init(uint32_t device_mask, cordahip_ctx** out);
void cordahip_shutdown(cordahip_ctx* ctx);
int cordahip_device_count(const cordahip_ctx* ctx);

/* Device memory (ABI 4). cordahip_device_mem: the bytes the library holds on
 * `device`'s GPU now and at most so far (workspaces, stages, fixed tables), and
 * its budget. The two byte counts are per GPU and process-wide: every context
 * on that GPU adds to them. The budget (CORDAHIP_DEVICE_MEM_BUDGET at
 * cordahip_init, bytes with an optional K/M/G suffix; default 128 GiB, at most 90% of the device)
 * sizes the verification workspaces -- Ed25519 45% (+20% for the pipelines'
 * second slot), ECDSA 15%; a smaller budget only costs extra launches. The
 * batch-proportional buffers (stages, id buffers) follow the batches. Buffers
 * are grow-only while a device is busy; after CORDAHIP_IDLE_RELEASE_MS (default
 * 30000; 0: never) without a call they are released, as cordahip_trim does now
 * (it waits for the calls in progress). INTEGRATION.md §6. */
int cordahip_device_mem(cordahip_ctx* ctx, int device, uint64_t* in_use, uint64_t* peak, uint64_t* budget);
int cordahip_trim(cordahip_ctx* ctx);

int cordahip_alloc_pinned(cordahip_ctx* ctx, size_t bytes, void** host);
int cordahip_free_pinned(cordahip_ctx* ctx, void* host);

/* ---- generic signature batch (host memory) ------------------------------ *
 * Variable-length fields are CSR: item i's key is key[key_off[i] .. key_off[i+1]).
 * Every CSR array in this header is CHECKED (ABI 4): offsets non-decreasing, the
 * last one within the buffer length the batch declares (key_bytes, sig_bytes,
 * msg_bytes, leaf_bytes_len, n_items, ntok), and each level's range inside the
 * next level's declared count (a transaction's leaves < nleaves, items < n_items,
 * signatures < nsig): the library reads no array past the entries its declared
 * count implies ([n+1] offsets for n entries). A violation fails the batch
 * with CORDAHIP_ERR_INVALID_ARG, never a read outside the caller's buffers:
 * transaction-level batches are checked whole before anything is enqueued; a
 * generic signature batch is checked lane by lane as its chunks are classified
 * (earlier chunks may then have written their statuses; the result is the error).
 * The context stays usable after INVALID_ARG.
 * Key encodings: Ed25519 = the 32-byte A (Kryo wire form, Kryo.kt:386); ECDSA =
 * SEC1 point (the SPKI BIT STRING payload, Crypto.kt:348-355).
 * verdict (optional): bit (i % 64) of word (i / 64) = (status[i] == OK).
 * flags: 0 = Crypto.doVerify semantics (Crypto.kt:472-483: empty signature or
 * clear data -> EMPTY); CORDAHIP_FLAG_IS_VALID = Crypto.isValid semantics
 * (Crypto.kt:534-541: no emptiness checks; an empty clear data is hashed like
 * any other message and may verify, an empty signature is MALFORMED_SIG at the
 * engine). Lanes are sharded over every context device (contiguous, 64-aligned
 * shards of each scheme's lanes; cordahip_shard_range).
 * CORDAHIP_FLAG_RSA_ON_DEVICE (may be or-ed in): RSA_SHA256 lanes are verified
 * on the GPU instead of answered UNSUPPORTED. The scheme is RSASSA-PSS
 * ("SHA256WITHRSAANDMGF1", Crypto.kt:77-88: SHA-256, MGF1-SHA-256, salt 32,
 * trailer 0xBC) by BouncyCastle 1.57's PSSSigner rules (parity
 * unpinned). The key is the SPKI BIT STRING payload, DER RSAPublicKey ::=
 * SEQUENCE { modulus INTEGER, publicExponent INTEGER }, decoded strictly:
 * anything else, or n <= 0 / e <= 0, is BAD_KEY. A key that decodes and that
 * the GPU path declines is UNSUPPORTED and stays with the JVM: an even modulus,
 * a modulus outside 1024..4096 bits, an even e, e < 3, e >= 2^32. Then EMPTY
 * (doVerify rules only); every other failure is BAD_SIG (the PSS engine never
 * throws, so MALFORMED_SIG does not occur for this scheme). Without the flag
 * such lanes are UNSUPPORTED as before, and a context that never sees it
 * allocates nothing for them. The signed-transaction and streaming entry
 * points have no flags: RSA lanes there stay UNSUPPORTED.                     */
#define CORDAHIP_FLAG_IS_VALID 1u
#define CORDAHIP_FLAG_RSA_ON_DEVICE 2u
typedef struct {
  uint64_t n;
  const uint8_t* scheme; /* [n] CORDAHIP_SCHEME_* */
  const uint8_t* key;
  const uint64_t* key_off; /* [n+1] */
  const uint8_t* sig;
  const uint64_t* sig_off; /* [n+1] */
  const uint8_t* msg;
  const uint64_t* msg_off; /* [n+1] */
  uint8_t* status;         /* [n] out */
  uint64_t* verdict;       /* [(n+63)/64] out, may be NULL */
  uint32_t flags;          /* CORDAHIP_FLAG_* */
  uint64_t key_bytes;      /* ABI 4: bytes at key; key_off[n] <= key_bytes */
  uint64_t sig_bytes;      /* bytes at sig */
  uint64_t msg_bytes;      /* bytes at msg */
} cordahip_sig_batch;

/* Tickets: every *_submit queues the batch on the context's worker pool and
 * returns at once. cordahip_wait() returns the batch's result code and RELEASES
 * the ticket (a second wait gives CORDAHIP_ERR_UNKNOWN_TICKET); cordahip_poll()
 * only reports progress, so every ticket must be waited on once (shutdown
 * waits for and releases the rest). The descriptor is copied at submit; the
 * buffers it points to stay the caller's and must stay untouched until wait. */
int cordahip_sig_submit(cordahip_ctx* ctx, const cordahip_sig_batch* batch, uint64_t* ticket);
/* timeout_ns < 0: wait forever; CORDAHIP_ERR_TIMEOUT keeps the ticket. */
int cordahip_wait(cordahip_ctx* ctx, uint64_t ticket, int64_t timeout_ns);
/* 1 = done (result retrievable with wait), 0 = pending, < 0 = error */
int cordahip_poll(cordahip_ctx* ctx, uint64_t ticket);
/* synchronous submit + wait */
int cordahip_sig_verify(cordahip_ctx* ctx, const cordahip_sig_batch* batch);

/* ---- dense Ed25519 paths -------------------------------------------------- *
 * keys n*32 B, sigs n*64 B (R || S), msgs n*msg_len B, all row-major.
 * _device: pointers are device (HBM) memory on `device`; 16-byte aligned;
 *          enqueued on hip_stream (a hipStream_t; NULL = the device's null
 *          stream, with HIP's usual null-stream ordering); asynchronous w.r.t.
 *          the host, ordered after earlier work on that stream.
 * _host:   host pointers (pinned recommended); shards over all context devices,
 *          pipelines H2D copy / kernel / D2H copy in chunks; synchronous.   */
int cordahip_ed25519_verify_device(cordahip_ctx* ctx, int device, const void* d_keys, const void* d_sigs,
                                   const void* d_msgs, uint32_t msg_len, uint64_t n, void* d_status,
                                   void* d_verdict, void* hip_stream);
int cordahip_ed25519_verify_host(cordahip_ctx* ctx, const uint8_t* keys, const uint8_t* sigs, const uint8_t* msgs,
                                 uint32_t msg_len, uint64_t n, uint8_t* status, uint64_t* verdict);

/* ---- dense ECDSA path (secp256k1 = 2 and P-256 = 3 mixed) ------------------ *
 * scheme[n]; keys in 65-byte slots (SEC1 04||X||Y or 02/03||X) + key_len[n];
 * DER signatures in 72-byte slots + sig_len[n] (72 = the longest DER encoding of
 * r, s < 2^256); msgs n*msg_len. Device memory; lanes are partitioned by curve on
 * the device (one curve per wavefront), status and verdict come back in input order.
 * A lane with sig_len > 72 does not fit its slot: it is MALFORMED_SIG here (EMPTY
 * first under doVerify rules), without reading past the slot. BouncyCastle would
 * say BAD_SIG for such a signature when its DER is well formed (an INTEGER of more
 * than 33 bytes is >= n): use the generic batch (cordahip_sig_verify), which
 * decides those lanes by the DER rules, for BC parity on over-long signatures. */
int cordahip_ecdsa_verify_device(cordahip_ctx* ctx, int device, const void* d_scheme, const void* d_keys,
                                 const void* d_key_len, const void* d_sigs, const void* d_sig_len, const void* d_msgs,
                                 uint32_t msg_len, uint64_t n, void* d_status, void* d_verdict, void* hip_stream);

/* ---- dense RSA paths (device memory on `device`, enqueued on hip_stream) ------ *
 * Rows of mod_words = 64, 96 or 128 little-endian uint32 words (moduli of up to
 * 2048 / 3072 / 4096 bits, zero-padded to the row), one width per call; other
 * widths are CORDAHIP_ERR_INVALID_ARG. d_exp: uint32[n]. Pointers 4-byte aligned.
 *
 * cordahip_rsa_public_op_device: out = in^e mod n per row, the raw public
 * operation (a caller can build PKCS#1 v1.5 certificate checks on it). The
 * call requires an odd modulus, e >= 1 and in < modulus; a row that violates
 * this yields a ZERO ROW. d_out may be d_in.
 *
 * cordahip_rsa_pss_verify_device: RSASSA-PSS verification (the rules of
 * CORDAHIP_FLAG_RSA_ON_DEVICE above), shaped like cordahip_ecdsa_verify_device:
 * signatures big-endian in 4*mod_words-byte slots + sig_len[n] (uint16),
 * messages n*msg_len. Statuses by doVerify rules (EMPTY for an empty signature
 * or msg_len 0). A sig_len beyond the slot is BAD_SIG without reading past the
 * slot (such a signature is longer than the modulus: parity-exact). Rows whose
 * modulus is even or below 1024 bits, or whose exponent is even or below 3,
 * are UNSUPPORTED. d_verdict may be NULL. */
int cordahip_rsa_public_op_device(cordahip_ctx* ctx, int device, const void* d_mod, const void* d_exp,
                                  const void* d_in, uint32_t mod_words, uint64_t n, void* d_out, void* hip_stream);
int cordahip_rsa_pss_verify_device(cordahip_ctx* ctx, int device, const void* d_mod, const void* d_exp,
                                   const void* d_sigs, const void* d_sig_len, const void* d_msgs, uint32_t msg_len,
                                   uint32_t mod_words, uint64_t n, void* d_status, void* d_verdict, void* hip_stream);

/* ---- the generic batch resident in device memory (K23) ------------------------- *
 * cordahip_sig_verify for a batch that already sits in HBM: scheme[n], the keys and
 * signatures as CSR (d_key_off / d_sig_off: uint64[n + 1], 8-byte aligned; the byte
 * buffers at any alignment, key_bytes / sig_bytes their declared sizes) and the
 * messages as msg_rows dense rows of msg_len bytes. d_msg_row (uint32[n], or NULL:
 * lane i signs row i) says which row a lane signs, so many signatures may share one
 * row (a transaction's id) without a copy per lane. The batch is classified and
 * packed into the verifiers' dense rows on the GPU, by the rule of cordahip_sig_verify
 * lane for lane, each family's generic verifier runs over its rows only, and the
 * statuses come back in lane order: enqueued on hip_stream, asynchronous to the host,
 * nothing read back. flags: CORDAHIP_FLAG_IS_VALID and / or CORDAHIP_FLAG_RSA_ON_DEVICE
 * with the meanings of cordahip_sig_batch; without the latter RSA_SHA256 lanes are
 * UNSUPPORTED and no RSA memory is allocated. d_verdict (uint64[(n + 63) / 64], bit =
 * status OK) may be NULL. Registered keys are not consulted: the call runs the generic
 * verifiers whatever cordahip_vkey_set_routing* say, unless
 * cordahip_vkey_set_routing_device is on.
 *
 * The host cannot see the offsets, so what is CORDAHIP_ERR_INVALID_ARG for a host batch
 * is a per-lane status here, as CORDAHIP_TX_BAD_COVER is for cordahip_tx_cover_device:
 * a lane whose key or signature range is reversed or reaches past key_bytes / sig_bytes,
 * or whose message row is >= msg_rows, gets CORDAHIP_STATUS_BAD_RANGE, and not one byte
 * of it is read. (The value is parenthesised like the error codes: the six statuses at
 * the top are Crypto.kt's, this one exists for device-resident batches only.)
 * Key ranges may overlap (many lanes over one key's bytes). The RSA rows are sized from
 * key_bytes (a key of 1024..2048 / ..3072 / ..4096 bits takes more than 131 / 260 / 388
 * bytes), so with overlapping ranges a width class can hold more RSA lanes than rows: the
 * lanes past key_bytes / 131 (260, 388) of their class, in lane order, are
 * CORDAHIP_STATUS_BAD_RANGE too. Disjoint ranges never meet this.
 * n >= 2^31 is CORDAHIP_ERR_INVALID_ARG (row indices are 32-bit). Scratch is per device
 * and grow-only (about 330 + 2 msg_len bytes a lane; with the RSA flag up to
 * key_bytes / 131 rows of 1.1 KB and fewer, wider ones), released by cordahip_trim. */
#define CORDAHIP_STATUS_BAD_RANGE (19)
int cordahip_sig_verify_device(cordahip_ctx* ctx, int device, const void* d_scheme, const void* d_key,
                               const void* d_key_off, uint64_t key_bytes, const void* d_sig, const void* d_sig_off,
                               uint64_t sig_bytes, const void* d_msgs, uint32_t msg_len, const void* d_msg_row,
                               uint64_t msg_rows, uint64_t n, uint32_t flags, void* d_status, void* d_verdict,
                               void* hip_stream);

/* ---- streaming mixed-scheme drain (verifier-module queue) ----- *
 * Replaces the per-request Crypto.isValid calls a verifier would make for a
 * queue of mixed-scheme requests (Crypto.kt:534-541; the out-of-process
 * verifier's request loop, verifier/.../Verifier.kt:58-75).
 * The producer writes requests straight into the two dense host layouts
 * (pinned memory from cordahip_alloc_pinned, or the copies are not
 * asynchronous): an Ed25519 section (as cordahip_ed25519_verify_host) and an
 * ECDSA section (as cordahip_ecdsa_verify_device, 65/72-byte slots). Each
 * context device takes a contiguous shard of both sections and streams it in
 * chunks of up to 2^23 lanes through 3 device buffer sets on three HIP
 * streams (every H2D on one copy stream; each section's kernels and status
 * D2H on its own stream, so a chunk's ECDSA kernels run beside its Ed25519
 * kernels), so the H2D copy of chunk k+1, the kernels of chunk k and the
 * status D2H of chunk k-1 overlap. All of the batch's host buffers, statuses
 * included, must be pinned. Synchronous; statuses land in ed_status /
 * ec_status.                                                                  */
typedef struct {
  uint64_t n_ed;
  const uint8_t* ed_keys; /* [n_ed*32] */
  const uint8_t* ed_sigs; /* [n_ed*64] */
  const uint8_t* ed_msgs; /* [n_ed*ed_msg_len] */
  uint32_t ed_msg_len;
  uint8_t* ed_status;     /* [n_ed] out */
  uint64_t n_ec;
  const uint8_t* ec_scheme;  /* [n_ec] 2 or 3 */
  const uint8_t* ec_keys;    /* [n_ec*65] SEC1 in 65-byte slots */
  const uint8_t* ec_key_len; /* [n_ec] */
  const uint8_t* ec_sigs;    /* [n_ec*72] DER in 72-byte slots */
  const uint8_t* ec_sig_len; /* [n_ec] */
  const uint8_t* ec_msgs;    /* [n_ec*ec_msg_len] */
  uint32_t ec_msg_len;
  uint8_t* ec_status;        /* [n_ec] out */
} cordahip_stream_batch;
int cordahip_stream_verify(cordahip_ctx* ctx, const cordahip_stream_batch* batch);

/* RFC 8032 keygen + sign from 32-byte seeds (device memory): corpus generation. */
int cordahip_ed25519_sign_device(cordahip_ctx* ctx, int device, const void* d_seeds, const void* d_msgs,
                                 uint32_t msg_len, uint64_t n, void* d_pubs, void* d_sigs, void* hip_stream);

/* ---- Ed25519 batch signing with registered keys -------------------------------- *
 * Replaces, per lane, Crypto.doSign(EDDSA_ED25519_SHA512, key, clearData)
 * (Crypto.kt:394-401) as the notary (NotaryFlow.Service.signAndSendResponse ->
 * service.sign(txId.bytes), NotaryFlow.kt:114-116), an oracle
 * (keyManagementService.sign(ftx.rootHash.bytes, key), NodeInterestRates.kt:149-180)
 * and ServiceHub.kt:138,179 reach it: a handful of long-lived keys, many 32-byte
 * ids. Ed25519 signing is deterministic (RFC 8032; i2p EdDSAEngine), so every
 * signature is bit-identical to the JVM's. ECDSA and RSA signing with registered
 * keys are the two sections after this one; CompositeSignature assembly is not
 * offered.
 *
 * Key registry. cordahip_signer_add_ed25519 expands the 32-byte seed on every
 * device of the context (h = SHA-512(seed), a = clamp(h[0:32]) mod L, prefix =
 * h[32:64], A = [a]B) into a 128-byte record of a per-device table, returns the
 * key's id and writes A (EdDSAPublicKey.Abyte, what the oracle's keypair gives)
 * to pub. A context holds up to 4096 live keys; a full table is
 * CORDAHIP_ERR_OUT_OF_MEMORY. The table (512 KB per device) is allocated by the
 * first add -- a context that never signs allocates nothing -- is counted in
 * cordahip_device_mem, and is kept by cordahip_trim and the idle release.
 * Custody: the seed crosses to each device through page-locked staging the
 * library wipes before add returns, and a device scratch the expansion kernel
 * zeroes; after add returns the host side holds no seed, a or prefix.
 * cordahip_signer_remove and cordahip_shutdown zero the record on every device
 * before they return (shutdown: before the table is freed). CORDAHIP_TRACE
 * never prints key material. INTEGRATION.md (key custody) says what this does
 * and does not protect against.
 * Ordering: remove waits for every signing call already enqueued on the
 * context's devices (caller streams included) before it zeroes the record, so
 * such a call signs with the key or not at all; a signing call enqueued after
 * remove returns answers CORDAHIP_SIGN_UNKNOWN_KEY for that id -- also after
 * the slot has been given to a new key: an id is never reused (slot | reuse
 * counter << 12, compared with the id stored in the record). remove of an id
 * that is not live is CORDAHIP_ERR_INVALID_ARG.
 *
 * Per-lane statuses, by precedence:
 *   CORDAHIP_SIGN_SKIPPED      gate[i] != 0 (the lane was not to be signed)
 *   CORDAHIP_SIGN_UNKNOWN_KEY  key_id[i] names no live key (the KMS looks the key
 *                              pair up before doSign, PersistentKeyManagementService.kt:87-89)
 *   CORDAHIP_STATUS_EMPTY      an empty message ("Signing of an empty array is
 *                              not permitted!", Crypto.kt:397)
 *   CORDAHIP_STATUS_OK         sig[i*64 .. i*64+64) = R || S
 * Every lane that is not OK gets 64 zero bytes; no secret is read for it.
 *
 * cordahip_sign / cordahip_sign_submit: host memory, messages CSR (checked as
 * every CSR array of this header is: msg_off non-decreasing within msg_bytes,
 * whole, before any enqueue; a single message of 2^32 bytes or more is refused
 * the same way: CORDAHIP_ERR_INVALID_ARG, outputs untouched, context usable).
 * Lanes are sharded over the context's devices (cordahip_shard_range, align 64)
 * and stream in chunks of CORDAHIP_HOST_CHUNK lanes through page-locked staging;
 * signature rows come back in lane order. */
#define CORDAHIP_SIGN_UNKNOWN_KEY 14
#define CORDAHIP_SIGN_SKIPPED 15
int cordahip_signer_add_ed25519(cordahip_ctx* ctx, const uint8_t seed[32], uint32_t* key_id, uint8_t pub[32]);
int cordahip_signer_remove(cordahip_ctx* ctx, uint32_t key_id);
typedef struct {
  uint64_t n;
  const uint32_t* key_id;  /* [n] ids from cordahip_signer_add_ed25519 */
  const uint8_t* msg;
  const uint64_t* msg_off; /* [n+1] into msg */
  const uint8_t* gate;     /* [n] nonzero: skip the lane; may be NULL */
  uint8_t* sig;            /* [n*64] out: R || S, zero rows for lanes that are not OK */
  uint8_t* status;         /* [n] out */
  uint64_t msg_bytes;      /* bytes at msg; msg_off[n] <= msg_bytes */
} cordahip_sign_batch;
int cordahip_sign(cordahip_ctx* ctx, const cordahip_sign_batch* batch);
int cordahip_sign_submit(cordahip_ctx* ctx, const cordahip_sign_batch* batch, uint64_t* ticket);
/* Device-resident form: d_key_id uint32[n], d_msgs dense rows of msg_len bytes
 * (16-byte aligned when msg_len == 32, the one-block shape), d_gate uint8[n] or
 * NULL, d_sigs [n*64] (16-byte aligned), d_status [n], all in HBM on `device`,
 * on hip_stream. d_gate is typically the tx_status an earlier call on the same
 * stream wrote (cordahip_filtered_tx_verify's kernels, a *_device signed-tx
 * call): "verify, then sign only what verified" without a host round trip.
 * msg_len == 0 makes every ungated lane with a live key EMPTY. */
int cordahip_ed25519_sign_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_msgs,
                                       uint32_t msg_len, uint64_t n, const void* d_gate, void* d_sigs,
                                       void* d_status, void* hip_stream);

/* ---- ECDSA batch signing with registered keys (RFC 6979 nonces) ----------------- *
 * Replaces, per lane, Crypto.doSign(ECDSA_SECP256K1_SHA256 / ECDSA_SECP256R1_SHA256,
 * key, clearData) (Crypto.kt:394-401 -> JCA "SHA256withECDSA") for a notary, oracle or
 * issuer whose identity key is an ECDSA key. BouncyCastle's default signer draws a
 * random nonce, so no implementation can reproduce the JVM's bytes; an ECDSA
 * signature is judged by its verifier, and this signer derives the nonce as RFC 6979
 * 3.2 does (HMAC-SHA256; BouncyCastle ships the same rule as HMacDSAKCalculator):
 * reproducible, no random number generator on the GPU, and accepted by every
 * verifier, Crypto.doVerify included. Per lane:
 *   h1 = SHA-256(m), e = int(h1) mod n, k = the RFC 6979 nonce of (d, h1),
 *   r = x([k]G) mod n, s = k^-1 (e + d r) mod n,
 *   sig = the minimal DER SEQUENCE { INTEGER r, INTEGER s } in a 72-byte slot.
 * s is not normalised to the low half (BC 1.57 does not normalise it either, nor do
 * the RFC's vectors). A candidate with k = 0, k >= n, r = 0 or s = 0 is passed over
 * by the RFC's 3.2 h.3 update; the loop is bounded at 8 candidates, and a lane that
 * exhausts it answers CORDAHIP_SIGN_FAILED with a zero row -- for a correct
 * implementation an event of probability below 2^-250 on either curve (a candidate is
 * rejected with probability below 2^-31: n > 2^256 - 2^225 on P-256 and
 * n > 2^256 - 2^129 on secp256k1, and r = 0 or s = 0 needs a 2^-256 coincidence;
 * eight in a row: below 2^-250).
 *
 * Key registry. cordahip_signer_add_ecdsa takes the private scalar d as 32 big-endian
 * bytes. d = 0 or d >= n is data, not an ABI error: CORDAHIP_SUCCESS with
 * *key_status = CORDAHIP_STATUS_BAD_KEY, *key_id = 0xFFFFFFFF and no slot taken; a
 * scheme other than 2 or 3 is CORDAHIP_ERR_INVALID_ARG. Otherwise a kernel on every
 * device writes the key's record and pub receives Q = [d]G as 65 SEC1 uncompressed
 * bytes. Ids come from the signer's one pool (4096 slots with the Ed25519 keys, the
 * same id form), and cordahip_signer_remove serves both families with the ordering
 * stated above. An ECDSA id handed to cordahip_sign* answers
 * CORDAHIP_SIGN_UNKNOWN_KEY, and an Ed25519 id handed to cordahip_ecdsa_sign* does.
 * The ECDSA records and the two curves' comb tables [d 16^j]G (40 KiB each, built on
 * a device's first key of the curve) are an allocation of their own (592 KB per
 * device), made by the first ECDSA add, counted in cordahip_device_mem and kept by
 * cordahip_trim and the idle release. Custody is the Ed25519 signer's: d crosses
 * through page-locked staging wiped before add returns and a device scratch the add
 * kernel zeroes; remove and shutdown zero the record on every device;
 * CORDAHIP_TRACE never prints key material. The kernel reads no address and takes no
 * branch that depends on d, the nonce or their digits.
 *
 * Per-lane statuses, by precedence: CORDAHIP_SIGN_SKIPPED, CORDAHIP_SIGN_UNKNOWN_KEY,
 * CORDAHIP_STATUS_EMPTY (as for cordahip_sign), CORDAHIP_SIGN_FAILED, then
 * CORDAHIP_STATUS_OK: sig[i*72 .. i*72+sig_len[i]) is the signature, the rest of the
 * slot zero. Every lane that is not OK gets 72 zero bytes and length 0; no secret is
 * read for it. A batch may mix both curves and many keys.
 *
 * cordahip_ecdsa_sign / _submit: host memory, CSR checked whole before any enqueue,
 * sharding, CORDAHIP_HOST_CHUNK chunking and tickets as for cordahip_sign.
 *
 * CORDAHIP_SIGN_FAILED is an enumerator, not one of the CORDAHIP_SIGN_* macros: those
 * two are the statuses every signing call shares, and no other lane status has their
 * values. This one is the ECDSA signing calls' alone, and its value, 16, is also
 * CORDAHIP_VERIFY_UNKNOWN_KEY's (keyed verification) and CORDAHIP_COMMIT_CONFLICT's
 * (the commit log); no call writes two of them, so a status array is read by the call
 * that filled it. */
enum { CORDAHIP_SIGN_FAILED = 16 };
int cordahip_signer_add_ecdsa(cordahip_ctx* ctx, uint32_t scheme, const uint8_t d[32] /* big-endian */,
                              uint32_t* key_id, uint8_t* key_status, uint8_t pub[65]);
typedef struct {
  uint64_t n;
  const uint32_t* key_id;  /* [n] ids from cordahip_signer_add_ecdsa */
  const uint8_t* msg;
  const uint64_t* msg_off; /* [n+1] into msg */
  const uint8_t* gate;     /* [n] nonzero: skip the lane; may be NULL */
  uint8_t* sig;            /* [n*72] out: DER, zero-padded; zero rows for lanes that are not OK */
  uint8_t* sig_len;        /* [n] out */
  uint8_t* status;         /* [n] out */
  uint64_t msg_bytes;      /* bytes at msg; msg_off[n] <= msg_bytes */
} cordahip_ecdsa_sign_batch;
int cordahip_ecdsa_sign(cordahip_ctx* ctx, const cordahip_ecdsa_sign_batch* batch);
int cordahip_ecdsa_sign_submit(cordahip_ctx* ctx, const cordahip_ecdsa_sign_batch* batch, uint64_t* ticket);
/* Device-resident form: d_key_id uint32[n], d_msgs dense rows of msg_len bytes,
 * d_gate uint8[n] or NULL, d_sigs [n*72] (4-byte aligned), d_sig_len [n], d_status [n],
 * all in HBM on `device`, on hip_stream. d_gate is typically the tx_status an earlier
 * call on the same stream wrote. msg_len == 0 makes every ungated lane with a live
 * key EMPTY. */
int cordahip_ecdsa_sign_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_msgs,
                                     uint32_t msg_len, uint64_t n, const void* d_gate, void* d_sigs,
                                     void* d_sig_len, void* d_status, void* hip_stream);

/* ---- RSA_SHA256 batch signing with registered private keys (RSASSA-PSS) ---------- *
 * Replaces, per lane, Crypto.doSign(RSA_SHA256, key, clearData) (Crypto.kt:394-401 ->
 * JCA "SHA256WITHRSAANDMGF1" -> BouncyCastle PSSSigner.generateSignature) for a notary,
 * oracle or issuer whose identity key is an RSA key. BouncyCastle draws the 32-byte
 * salt from SecureRandom, so no implementation can reproduce the JVM's bytes; a
 * signature is judged by its verifier. Here the caller draws the salt of every lane
 * and passes it in: no random number generator on the GPU, and the output is a pure
 * function of (key, message, salt). Per lane, with key (n, e, p, q, dP, dQ, qInv):
 *   mHash = SHA-256(m), H = SHA-256(0x00 * 8 || mHash || salt),
 *   DB = 0x00 .. || 0x01 || salt (emLen - 33 bytes; emBits = bits(n) - 1,
 *   emLen = ceil(emBits / 8)), EM = (DB xor MGF1-SHA256(H)) with the bits above emBits
 *   cleared || H || 0xBC (RFC 8017 9.1.1),
 *   s = EM^d mod n by the CRT: m1 = EM^dP mod p, m2 = EM^dQ mod q,
 *   h = qInv (m1 - m2) mod p, s = m2 + q h (RFC 8017 5.1.2 2.b),
 *   sig = s as k = ceil(bits(n) / 8) big-endian bytes, left-padded with zeros (I2OSP).
 * PARITY UNPINNED, like every PSS rule of this header: neither BouncyCastle's sources
 * nor an RSA signature exist in the reference; the k-byte length is what RFC 8017 gives
 * and what BC's engine is believed to return. The signatures verify under
 * cordahip_sig_verify (CORDAHIP_FLAG_RSA_ON_DEVICE), cordahip_rsa_verify_keyed and
 * OpenSSL.
 * Before a signature leaves the device the kernel checks s^e mod n == EM with the key's
 * public half; a lane that fails answers CORDAHIP_SIGN_FAILED with a zero slot (a CRT
 * signature with one faulty half gives away a factor of n).
 *
 * Key registry. cordahip_signer_add_rsa takes the CRT components as big-endian
 * magnitudes (any leading zeros) and e = RSAPrivateCrtKey.publicExponent; the host
 * derives n = p q and the Montgomery constants. Ids come from the signer's one pool (the
 * same id form), and cordahip_signer_remove serves all three families with the ordering
 * stated above. A context holds at most CORDAHIP_RSA_SIGNER_MAX_KEYS live RSA signing
 * keys; one more is CORDAHIP_ERR_OUT_OF_MEMORY. Data, not ABI errors (CORDAHIP_SUCCESS,
 * *key_id = 0xFFFFFFFF, no slot taken):
 *   CORDAHIP_STATUS_UNSUPPORTED  what the GPU path declines: bits(n) outside 1024..4096,
 *                                or the larger prime above half the width class
 *                                (16 * mod_words bits: unbalanced primes)
 *   CORDAHIP_STATUS_BAD_KEY      a zero-length component; p or q even or < 3; p = q;
 *                                e even or < 3; dP >= p, dQ >= q or qInv >= p; or the
 *                                consistency run fails: every device signs a fixed EM with
 *                                the new record and checks it with (n, e), which catches a
 *                                dP, dQ or qInv that does not belong to p, q and e.
 * Primality is not checked. A NULL pointer is CORDAHIP_ERR_INVALID_ARG. On success
 * modulus receives n as k big-endian bytes (the rest of the 512 zero) and
 * *modulus_len = k; every device must agree. The RSA signer table (a slot -> record
 * index over the pool's 4096 slots and 64 records of 3360 bytes: 232,496 bytes per
 * device) is an allocation of its own, made by the first RSA add that reaches a device,
 * counted in cordahip_device_mem and kept by cordahip_trim and the idle release.
 * Custody is the other signers': the components cross through page-locked staging wiped
 * before add returns; the host keeps id, width class and bit length only; remove and
 * shutdown zero the record on every device; the kernel keeps m1, m2 and h in registers
 * and zeroes its LDS table before it ends; CORDAHIP_TRACE never prints key material. The
 * kernel reads no address and takes no branch that depends on p, q, dP, dQ, qInv, their
 * window digits or any intermediate mod p or mod q.
 *
 * Per-lane statuses, by precedence: CORDAHIP_SIGN_SKIPPED, CORDAHIP_SIGN_UNKNOWN_KEY (no
 * live RSA signer of that id -- also an Ed25519 or ECDSA signer id, and in the device
 * call a key of another width class; an RSA id handed to cordahip_sign* or
 * cordahip_ecdsa_sign* answers the same), CORDAHIP_STATUS_EMPTY, CORDAHIP_SIGN_FAILED,
 * then CORDAHIP_STATUS_OK: sig[i*512 .. i*512+sig_len[i]) is the signature, the rest of
 * the slot zero. Every lane that is not OK gets a zero slot and length 0; no secret is
 * read for it.
 *
 * cordahip_rsa_sign / _submit: host memory, CSR checked whole before any enqueue (a NULL
 * salt is CORDAHIP_ERR_INVALID_ARG, outputs untouched), sharding, CORDAHIP_HOST_CHUNK
 * chunking and tickets as for cordahip_sign; a chunk's lanes are grouped by their key's
 * width class and each class runs over its rows only. */
#define CORDAHIP_RSA_SIGNER_MAX_KEYS 64
#define CORDAHIP_RSA_SIG_SLOT 512
typedef struct {              /* big-endian magnitudes, any leading zeros */
  const uint8_t *p, *q, *dp, *dq, *qinv;
  uint32_t p_len, q_len, dp_len, dq_len, qinv_len;
  uint32_t e;                 /* RSAPrivateCrtKey.publicExponent */
} cordahip_rsa_private_key;
int cordahip_signer_add_rsa(cordahip_ctx* ctx, const cordahip_rsa_private_key* key, uint32_t* key_id,
                            uint8_t* key_status, uint8_t modulus[512], uint32_t* modulus_len);
typedef struct {
  uint64_t n;
  const uint32_t* key_id;  /* [n] ids from cordahip_signer_add_rsa */
  const uint8_t* msg;
  const uint64_t* msg_off; /* [n+1] into msg */
  const uint8_t* gate;     /* [n] nonzero: skip the lane; may be NULL */
  const uint8_t* salt;     /* [n*32], required */
  uint8_t* sig;            /* [n*512] out: k bytes at the start of the slot, rest zero */
  uint16_t* sig_len;       /* [n] out: k, or 0 */
  uint8_t* status;         /* [n] out */
  uint64_t msg_bytes;      /* bytes at msg; msg_off[n] <= msg_bytes */
} cordahip_rsa_sign_batch;
int cordahip_rsa_sign(cordahip_ctx* ctx, const cordahip_rsa_sign_batch* batch);
int cordahip_rsa_sign_submit(cordahip_ctx* ctx, const cordahip_rsa_sign_batch* batch, uint64_t* ticket);
/* Device-resident form, one width class per call (mod_words = 64 / 96 / 128 for moduli
 * of up to 2048 / 3072 / 4096 bits): d_key_id uint32[n], d_msgs dense rows of msg_len
 * bytes, d_salts [n*32], d_gate uint8[n] or NULL, d_sigs [n] slots of 4*mod_words
 * bytes, d_sig_len uint16[n], d_status [n], all in HBM on `device`, on hip_stream. d_gate
 * is typically the tx_status an earlier call on the same stream wrote. A key of another
 * class is CORDAHIP_SIGN_UNKNOWN_KEY; msg_len == 0 makes every ungated lane with a live
 * key EMPTY. */
int cordahip_rsa_sign_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_msgs,
                                   uint32_t msg_len, const void* d_salts, uint32_t mod_words, uint64_t n,
                                   const void* d_gate, void* d_sigs /* 4*mod_words-byte slots */,
                                   void* d_sig_len /* uint16[n] */, void* d_status, void* hip_stream);

/* ---- Ed25519 batch verification against registered public keys ----------------- *
 * Replaces, per lane, Crypto.doVerify / Crypto.isValid(EDDSA_ED25519_SHA512, key,
 * sig, clear) (Crypto.kt:472-541) for the keys a node sees all day: the notary
 * identities of the network map (every transaction ResolveTransactionsFlow walks
 * carries a notary signature; the client's check of the notary's answer,
 * NotaryFlow.kt:75-83), its oracles' keys, fixed issuers. A key is registered
 * once; a lane then names it by id and is verified as i2p's engine states the
 * rule, encode([S_eff]B + [h](-A)) == R bytewise, from tables alone (64 mixed
 * additions: signed 8-bit windows over the key's table and over one of B) -- no
 * key decompression, no doubling, no decode of R. Apart from UNKNOWN_KEY a lane
 * answers exactly what cordahip_sig_verify answers for the same signature and
 * message with that key's bytes, under both flags values.
 *
 * Key registry. cordahip_vkey_add_ed25519 decodes the 32 bytes by the rules the
 * generic path uses (i2p 0.2.0 GroupElement(curve, bytes): y not range checked,
 * x = 0 with the sign bit set accepted, no small-order check). Bytes that do
 * not decode are data, not an ABI error: the call returns CORDAHIP_SUCCESS with
 * *key_status = CORDAHIP_STATUS_BAD_KEY and *key_id = 0xFFFFFFFF and takes no
 * slot (the JVM raises at key construction, as today). Otherwise *key_status =
 * CORDAHIP_STATUS_OK and a kernel on every device of the context builds the
 * key's record: the canonical Abyte (what SHA-512 hashes) and the window table
 * [d 256^j](-A), d = 1..128, j = 0..31 (512 KiB). Two adds of the same bytes
 * give two ids. A context holds up to 64 live keys (CORDAHIP_VKEY_MAX_KEYS); a
 * full registry is CORDAHIP_ERR_OUT_OF_MEMORY. The tables (32.5 MiB per device:
 * 64 keys' and the base point's) are allocated by the first add -- a context that never registers a key
 * allocates nothing -- are counted in cordahip_device_mem, and are kept by
 * cordahip_trim and the idle release.
 * Ordering, as for the signer: cordahip_vkey_remove waits for every keyed call
 * already enqueued on the context's devices (caller streams included) before it
 * clears the record; a call enqueued after remove returns answers
 * CORDAHIP_VERIFY_UNKNOWN_KEY for that id -- also after the slot has been given
 * to a new key: an id is never reused (slot | reuse counter << 6, compared with
 * the id stored in the record). remove of an id that is not live is
 * CORDAHIP_ERR_INVALID_ARG.
 * Verification-key ids and signer ids (cordahip_signer_add_ed25519) are separate
 * namespaces: neither call accepts the other's ids.
 * A public key is public. No custody rule applies to these tables and nothing
 * about them is constant-time: the kernel gathers table entries indexed by a
 * lane's own digits (the signer's read-everything-and-select scan protects a
 * secret scalar; here it would only cost time).
 *
 * Per-lane statuses, by precedence:
 *   CORDAHIP_VERIFY_UNKNOWN_KEY   key_id[i] names no live key (no table is read)
 *   CORDAHIP_STATUS_EMPTY         flags == 0 (doVerify) only: empty signature or
 *                                 empty message (Crypto.kt:475-476)
 *   CORDAHIP_STATUS_MALFORMED_SIG signature length != 64
 *   CORDAHIP_STATUS_BAD_SIG
 *   CORDAHIP_STATUS_OK
 * verdict bit i = (status[i] == OK).
 *
 * cordahip_verify_keyed / cordahip_verify_keyed_submit: host memory, signatures
 * and messages CSR, checked whole before any enqueue (sig_off, msg_off
 * non-decreasing within sig_bytes, msg_bytes; a single message of 2^32 bytes or
 * more is refused the same way): CORDAHIP_ERR_INVALID_ARG, outputs untouched,
 * context usable. Lanes are sharded over the context's devices
 * (cordahip_shard_range, align 64: a device owns whole verdict words) and stream
 * in chunks of CORDAHIP_HOST_CHUNK lanes through page-locked staging. */
#define CORDAHIP_VERIFY_UNKNOWN_KEY 16
#define CORDAHIP_VKEY_MAX_KEYS 64 /* live keys per context */
int cordahip_vkey_add_ed25519(cordahip_ctx* ctx, const uint8_t key[32], uint32_t* key_id, uint8_t* key_status);
int cordahip_vkey_remove(cordahip_ctx* ctx, uint32_t key_id);
typedef struct {
  uint64_t n;
  const uint32_t* key_id;  /* [n] ids from cordahip_vkey_add_ed25519 */
  const uint8_t* sig;
  const uint64_t* sig_off; /* [n+1] into sig */
  const uint8_t* msg;
  const uint64_t* msg_off; /* [n+1] into msg */
  uint8_t* status;         /* [n] out */
  uint64_t* verdict;       /* [(n+63)/64] out, may be NULL */
  uint32_t flags;          /* 0 or CORDAHIP_FLAG_IS_VALID */
  uint64_t sig_bytes, msg_bytes; /* bytes at sig / msg; sig_off[n] <= sig_bytes, msg_off[n] <= msg_bytes */
} cordahip_keyed_sig_batch;
int cordahip_verify_keyed(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch);
int cordahip_verify_keyed_submit(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch, uint64_t* ticket);
/* Device-resident form, doVerify rules: d_key_id uint32[n], d_sigs dense 64-byte
 * rows, d_msgs dense rows of msg_len bytes (both 16-byte aligned, as for
 * cordahip_ed25519_verify_device), d_status [n], d_verdict [(n+63)/64] or NULL,
 * all in HBM on `device`, on hip_stream. msg_len == 0 makes every lane with a
 * live key EMPTY, as in cordahip_ed25519_verify_device. */
int cordahip_ed25519_verify_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_sigs,
                                         const void* d_msgs, uint32_t msg_len, uint64_t n, void* d_status,
                                         void* d_verdict, void* hip_stream);

/* ---- Routing registered-key lanes to the keyed verifier (kernel K14) ----------
 * The calls the JVM makes with mixed batches -- cordahip_sig_verify / _submit,
 * the signed-tx calls (host and device), cordahip_ed25519_verify_device / _host,
 * cordahip_stream_verify -- carry key bytes, not key ids. With routing on, the
 * library recognises the lanes of registered Ed25519 keys itself, on the GPU, and
 * verifies them with the keyed verifier above; the caller changes nothing else.
 *
 * cordahip_vkey_set_routing(ctx, on): on != 0 turns routing on for every device of
 * the context, 0 (the default) off. It takes effect with the next Ed25519 batch
 * enqueued. Off, every call does exactly what it did before this switch existed:
 * nothing more is launched, allocated or locked.
 *
 * The rule, while routing is on and the device holds at least one live Ed25519
 * verification key: a lane is verified by the keyed verifier exactly when its 32
 * key bytes equal the canonical encoding (EdDSAPublicKey.Abyte) stored in a live
 * record; every other lane by the generic verifier as before. Nothing but the key
 * bytes enters the decision. A non-canonical encoding of a registered point
 * misses and stays generic (which decodes it to the same point); of two live
 * records with equal bytes either may serve; ECDSA records are never matched
 * by this switch (ECDSA lanes have one of their own: cordahip_vkey_set_routing_ecdsa
 * below, kernel K15).
 * Every lane's status and verdict bit equal the unrouted call's under both flags
 * values; no lane of these calls ever answers CORDAHIP_VERIFY_UNKNOWN_KEY.
 * The partition runs on the caller's stream and the host reads no count back.
 * It needs 12 bytes per lane of scratch per Ed25519 workspace slot (grown in
 * powers of two from 2^16 lanes), counted in cordahip_device_mem and released by
 * cordahip_trim and the idle release with the workspace; a batch whose scratch
 * does not fit in device memory is verified unrouted, not failed. Batches of 2^32 lanes or more in one enqueue are not routed.
 *
 * Ordering: a routed batch is a keyed call. cordahip_vkey_remove waits for the
 * routed batches already enqueued before it clears a record, so no record dies
 * between a lane's match and its verification; an add or a remove that races a
 * batch decides only which verifier a lane takes, never its status.
 *
 * cordahip_vkey_route_stats: the lanes that routed enqueues on `device` have sent
 * to the keyed and to the generic verifier since cordahip_init. Lanes verified
 * while routing was off, or while the device held no live Ed25519 key, count in
 * neither. The call waits for the routed work already enqueued on the device. */
int cordahip_vkey_set_routing(cordahip_ctx* ctx, uint32_t on);
int cordahip_vkey_route_stats(cordahip_ctx* ctx, int device, uint64_t* keyed_lanes, uint64_t* generic_lanes);

/* ---- ECDSA verification against registered public keys (kernel K13) --------
 * Replaces, per lane, Crypto.doVerify / Crypto.isValid for ECDSA_SECP256K1_SHA256
 * (2) and ECDSA_SECP256R1_SHA256 (3) (Crypto.kt:472-541 -> BouncyCastle
 * ECDSASigner.verifySignature) for long-lived keys: notaries and oracles whose
 * keys sit in an HSM, the doorman's and the node CAs' certificate keys. A key is
 * registered once; a lane names it by id and computes P = [e/s]G + [r/s]Q from
 * window tables alone -- 64 mixed additions over signed 8-bit digits of the two
 * scalars, the key's table and one of the curve's base point -- then decides
 * x(P) mod n == r projectively: no doubling, no key decode (no square root for a
 * compressed key), no per-lane table, no workspace. Apart from UNKNOWN_KEY a lane
 * answers exactly what cordahip_sig_verify answers for the same signature and
 * message with that key's bytes, under both flags values.
 *
 * Key registry. cordahip_vkey_add_ecdsa decodes the SEC1 bytes by the rules the
 * generic path uses (BC ECCurve.decodePoint: uncompressed 04 || x || y or
 * compressed 02 / 03 || x; a wrong length, a hybrid or infinity encoding, x or
 * y >= p, a point off the curve, an x without a square root are not keys). Such
 * bytes are data, not an ABI error: CORDAHIP_SUCCESS with *key_status =
 * CORDAHIP_STATUS_BAD_KEY and *key_id = 0xFFFFFFFF, and no slot is taken. A
 * scheme other than 2 or 3 is CORDAHIP_ERR_INVALID_ARG. Otherwise a kernel on
 * every device of the context builds the key's record and its window table
 * [d 256^j]Q, d = 1..128, j = 0..31 (320 KiB).
 * The registry is the Ed25519 one: ONE pool of CORDAHIP_VKEY_MAX_KEYS live keys
 * per context and one id space for both families; the 65th live key of either
 * family is CORDAHIP_ERR_OUT_OF_MEMORY, and cordahip_vkey_remove removes a key
 * of either family, with the ordering documented above. An ECDSA id given to
 * cordahip_verify_keyed, or an Ed25519 id given to the calls below, names no key
 * of that family: the lane is CORDAHIP_VERIFY_UNKNOWN_KEY.
 * The ECDSA tables (20.6 MiB per device: 64 keys' and the two curves' base
 * points') are allocated by the first ECDSA add of 33 or 65 bytes, whether or
 * not the device then takes the bytes for a point (the decode runs there) -- a
 * context that calls only the Ed25519 add, or none, does not allocate them -- are counted in
 * cordahip_device_mem, and are kept by cordahip_trim and the idle release.
 * Nothing about them is constant-time: a public key is public.
 *
 * Per-lane statuses, by precedence:
 *   CORDAHIP_VERIFY_UNKNOWN_KEY   key_id[i] names no live ECDSA key (no table is read)
 *   CORDAHIP_STATUS_EMPTY         flags == 0 (doVerify) only: empty signature or
 *                                 empty message (Crypto.kt:475-476)
 *   CORDAHIP_STATUS_MALFORMED_SIG not strict DER (der.hpp rules)
 *   CORDAHIP_STATUS_BAD_SIG       r or s outside [1, n-1], or the equation fails
 *   CORDAHIP_STATUS_OK
 * verdict bit i = (status[i] == OK).
 *
 * cordahip_ecdsa_verify_keyed / _submit: cordahip_keyed_sig_batch with DER
 * signatures of any length in the CSR; checks, sharding, chunking and staging as
 * for cordahip_verify_keyed. A signature longer than 72 bytes holds no r, s < n:
 * the DER rules decide it on the host (BAD_SIG when well-formed, else
 * MALFORMED_SIG), exactly as for generic batches. */
int cordahip_vkey_add_ecdsa(cordahip_ctx* ctx, uint32_t scheme, const uint8_t* key, uint32_t key_len,
                            uint32_t* key_id, uint8_t* key_status);
int cordahip_ecdsa_verify_keyed(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch);
int cordahip_ecdsa_verify_keyed_submit(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch, uint64_t* ticket);
/* Device-resident form, doVerify rules: d_key_id uint32[n], d_sigs DER signatures in
 * dense 72-byte slots, d_sig_len uint8[n], d_msgs dense rows of msg_len bytes,
 * d_status [n], d_verdict [(n+63)/64] or NULL, all in HBM on `device`, on
 * hip_stream. As in cordahip_ecdsa_verify_device, a sig_len above 72 is
 * MALFORMED_SIG (EMPTY first when msg_len == 0), and msg_len == 0 makes every
 * lane with a live key EMPTY. */
int cordahip_ecdsa_verify_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_sigs,
                                       const void* d_sig_len, const void* d_msgs, uint32_t msg_len, uint64_t n,
                                       void* d_status, void* d_verdict, void* hip_stream);

/* ---- Routing registered-key ECDSA lanes to the keyed verifier (kernel K15) ----
 * What kernel K14 does for Ed25519 lanes, for ECDSA lanes and K13: the calls that
 * carry key bytes -- cordahip_sig_verify / _submit, the host signed-tx calls,
 * cordahip_ecdsa_verify_device, cordahip_stream_verify -- recognise the lanes of
 * registered ECDSA keys themselves, on the GPU, and verify them with the keyed
 * verifier above. A switch and counters of their own: cordahip_vkey_set_routing
 * and cordahip_vkey_route_stats keep their meaning and stay Ed25519-only.
 *
 * cordahip_vkey_set_routing_ecdsa(ctx, on): on != 0 turns ECDSA routing on for
 * every device of the context, 0 (the default) off. It takes effect with the next
 * ECDSA batch enqueued. Off, every call does exactly what it did before this
 * switch existed: nothing more is launched, allocated or locked (one relaxed
 * atomic load decides).
 *
 * The rule, while ECDSA routing is on and the device holds at least one live ECDSA
 * verification key: a lane is verified by the keyed verifier exactly when its
 * scheme is 2 or 3 and equals the scheme of a live ECDSA record, and its key bytes
 * are one of the two SEC1 encodings of that record's point: 65 bytes 04 || X || Y,
 * or 33 bytes (02 | Y's low bit) || X, X and Y canonical (below p), big-endian.
 * Nothing but the lane's scheme, key length and key bytes enters the decision.
 * Both accepted encodings of a registered point match; hybrid encodings are not
 * keys, so there is no third. Each of these misses and stays generic, which
 * answers exactly what it answers today: a lane of the other scheme with the same
 * bytes, 04 || X || p - Y (another point), 04 || X || Y + p (not a key), a
 * compressed encoding with the wrong parity (another point), any other length.
 * Of two live records of one scheme that hold the same point either may serve;
 * Ed25519 records are never seen. Every lane's status and verdict bit equal the
 * unrouted call's under both flags values (K13's own contract: it applies the
 * host's pre-status, the doVerify EMPTY rule and the sig_len > 72 rule as the
 * generic verifier does); no lane of these calls ever answers
 * CORDAHIP_VERIFY_UNKNOWN_KEY.
 * The partition runs on the caller's stream and the host reads no count back; the
 * keyed lanes run as one launch per curve over that curve's lanes only, so a batch
 * that mixes curves pays each curve's instance for its own lanes. It needs 4,672
 * bytes and 4 bytes per lane of scratch per ECDSA workspace slot (the lanes grown
 * in powers of two from 2^16), counted in cordahip_device_mem and released by
 * cordahip_trim and the idle release with the workspace, and 16 bytes of counters
 * per device, which are kept; the ECDSA key tables keep their size. A batch whose
 * scratch does not fit in device memory is verified unrouted, not failed, as is
 * one enqueued after the device's last ECDSA key was removed. Batches of 2^32
 * lanes or more in one enqueue are not routed.
 *
 * Ordering: a routed batch is a keyed call. cordahip_vkey_remove waits for the
 * routed batches already enqueued before it clears a record, so no record dies
 * between a lane's match and its verification; an add or a remove that races a
 * batch decides only which verifier a lane takes, never its status.
 *
 * cordahip_vkey_route_stats_ecdsa: the lanes that routed ECDSA enqueues on `device`
 * have sent to the keyed and to the generic verifier since cordahip_init. Lanes
 * verified while ECDSA routing was off, or while the device held no live ECDSA
 * key, count in neither. The call waits for the routed work already enqueued on
 * the device. A device the context does not have is CORDAHIP_ERR_INVALID_ARG. */
int cordahip_vkey_set_routing_ecdsa(cordahip_ctx* ctx, uint32_t on);
int cordahip_vkey_route_stats_ecdsa(cordahip_ctx* ctx, int device, uint64_t* keyed_lanes, uint64_t* generic_lanes);

/* ---- RSA_SHA256 verification against registered public keys (kernel K18) -----
 * Replaces, per lane, Crypto.doVerify / Crypto.isValid(RSA_SHA256, key, sig, clear)
 * (Crypto.kt:472-541 -> BouncyCastle PSSSigner.verifySignature; the rules of
 * CORDAHIP_FLAG_RSA_ON_DEVICE above) for the RSA keys a network keeps for years:
 * TLS and legacy identity keys, certificate keys. A generic RSA lane derives its
 * key's Montgomery constants again on the device (n', R^2 mod n by doublings and
 * squarings, a conversion in and one out: 12 of the 29 modular products of a
 * 3072-bit, e = 65537 verification) and its host side parses the key's DER and
 * ships the modulus for every lane. A registered key keeps n' and one constant,
 * K = R^e mod n (R = 2^(32 words)): a lane names the key by id and computes
 * s^e mod n as the square-and-multiply chain over the UNCONVERTED signature
 * followed by one product with K -- 18 products for e = 65537, 3 for e = 3 --
 * then applies the PSS rules as the generic path does. Apart from UNKNOWN_KEY a
 * lane answers exactly what cordahip_sig_verify with CORDAHIP_FLAG_RSA_ON_DEVICE
 * answers for the same signature and message with that key's bytes, under both
 * flags values.
 *
 * Key registry. cordahip_vkey_add_rsa takes the SPKI BIT STRING payload (DER
 * RSAPublicKey), exactly what a generic batch lane carries, and decodes it by the
 * generic path's rules. Bytes that do not decode are data, not an ABI error:
 * CORDAHIP_SUCCESS with *key_status = CORDAHIP_STATUS_BAD_KEY, or
 * CORDAHIP_STATUS_UNSUPPORTED for a key BouncyCastle accepts and the GPU path
 * declines (even n, a modulus outside 1024..4096 bits, even e, e < 3, e >= 2^32)
 * -- the statuses a generic lane with that key gets -- with *key_id = 0xFFFFFFFF
 * and no slot taken. A NULL pointer is CORDAHIP_ERR_INVALID_ARG. Otherwise the
 * host builds the key's record (id, e, bit length, width class, n', n, K: 1,056
 * bytes) and copies it to every device of the context; no kernel runs.
 * The registry is the Ed25519 / ECDSA one: ONE pool of CORDAHIP_VKEY_MAX_KEYS live
 * keys per context and one id space for all three families; the 65th live key of
 * any family is CORDAHIP_ERR_OUT_OF_MEMORY, and cordahip_vkey_remove removes a
 * key of any family, with the ordering documented above (it waits for the RSA
 * table's fence; an id is never reused). An RSA id given to cordahip_verify_keyed
 * or cordahip_ecdsa_verify_keyed*, or an Ed25519 / ECDSA id given to the calls
 * below, names no key of that family: the lane is CORDAHIP_VERIFY_UNKNOWN_KEY.
 * The RSA table (64 records, 67,584 bytes per device) is allocated by a device's
 * first RSA add that decodes -- a context that never registers an RSA key does
 * not allocate it -- is counted in cordahip_device_mem, and is kept by
 * cordahip_trim and the idle release. A public key is public: nothing here is
 * constant-time.
 *
 * Per-lane statuses, by precedence:
 *   CORDAHIP_VERIFY_UNKNOWN_KEY   key_id[i] names no live RSA key (device calls:
 *                                 none of the call's width class); no record field
 *                                 beyond the id and the class is read
 *   CORDAHIP_STATUS_EMPTY         flags == 0 (doVerify) only: empty signature or
 *                                 empty message (Crypto.kt:475-476)
 *   CORDAHIP_STATUS_BAD_SIG       signature longer than the modulus, s >= n, or a
 *                                 PSS rule fails
 *   CORDAHIP_STATUS_OK
 * verdict bit i = (status[i] == OK).
 *
 * cordahip_rsa_verify_keyed / _submit: cordahip_keyed_sig_batch with big-endian
 * signatures of any length in the CSR; checks and sharding as for
 * cordahip_verify_keyed. A device's lanes stream a chunk of CORDAHIP_HOST_CHUNK
 * lanes at a time; a chunk's lanes are grouped by their key's width class (64, 96
 * or 128 words: moduli of up to 2048, 3072, 4096 bits) and each class present
 * runs over its rows only, 2^15 rows a launch; statuses and verdict words land in
 * lane order.
 *
 * Device-resident forms, doVerify rules, one width class per call like the dense
 * RSA calls (mod_words 64, 96 or 128, else CORDAHIP_ERR_INVALID_ARG): a live RSA
 * key of another class is UNKNOWN_KEY. cordahip_rsa_verify_keyed_device:
 * d_key_id uint32[n], d_sigs big-endian in 4*mod_words-byte slots, d_sig_len
 * uint16[n], d_msgs dense rows of msg_len bytes, d_status [n], d_verdict
 * [(n+63)/64] or NULL, all in HBM on `device`, on hip_stream. msg_len == 0 makes
 * every lane with a live key EMPTY; a sig_len beyond the slot is BAD_SIG without
 * reading past it. On a device where no RSA key was ever added every lane is
 * UNKNOWN_KEY.
 * cordahip_rsa_public_op_keyed_device is the kernel on its own: d_in / d_out rows
 * of mod_words little-endian uint32 words (4-byte aligned; d_out may be d_in),
 * out = in^e mod n of the lane's key; a ZERO ROW for an unknown key (or one of
 * another class) and for in >= n. */
int cordahip_vkey_add_rsa(cordahip_ctx* ctx, const uint8_t* key, uint32_t key_len, uint32_t* key_id,
                          uint8_t* key_status);
int cordahip_rsa_verify_keyed(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch);
int cordahip_rsa_verify_keyed_submit(cordahip_ctx* ctx, const cordahip_keyed_sig_batch* batch, uint64_t* ticket);
int cordahip_rsa_verify_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_sigs,
                                     const void* d_sig_len /* uint16[n] */, const void* d_msgs, uint32_t msg_len,
                                     uint32_t mod_words, uint64_t n, void* d_status, void* d_verdict,
                                     void* hip_stream);
int cordahip_rsa_public_op_keyed_device(cordahip_ctx* ctx, int device, const void* d_key_id, const void* d_in,
                                        uint32_t mod_words, uint64_t n, void* d_out, void* hip_stream);

/* ---- Routing registered-key RSA rows to the keyed exponentiation (kernel K20) ----
 * What kernels K14 and K15 do for Ed25519 and ECDSA lanes, for RSA rows and K18:
 * the calls that carry key bytes -- cordahip_rsa_pss_verify_device, the RSA
 * section of cordahip_sig_verify / _submit with CORDAHIP_FLAG_RSA_ON_DEVICE and the
 * RSA lanes of the signed-tx host calls (cordahip_set_rsa_on_device below) --
 * recognise the rows of registered RSA keys themselves, on the GPU, and run K18's
 * 18 modular products on them where the generic kernel runs 29 to 31. A switch and
 * counters of their own: the Ed25519 and ECDSA switches and counters keep their
 * meaning.
 *
 * cordahip_vkey_set_routing_rsa(ctx, on): on != 0 turns RSA routing on for every
 * device of the context, 0 (the default) off. It takes effect with the next RSA
 * enqueue. Off, every call does exactly what it did before this switch existed:
 * nothing more is launched, allocated or locked (one relaxed atomic load decides).
 *
 * The rule, while RSA routing is on and the device holds at least one live RSA
 * verification key: a row of a launch of width class W (mod_words) is keyed exactly
 * when some live RSA record has width class W, the row's exponent and the row's W
 * modulus words. Nothing else enters the decision. A registered 2048-bit key whose
 * modulus sits zero-padded in a 96- or 128-word row misses (its class is 64) and
 * stays generic, which answers exactly what it answers today, as does the registered
 * modulus under another exponent. Of two live records of one key either may serve.
 * The row still carries its modulus, so the generic prep and check kernels serve
 * every row unchanged -- the bit length, the UNSUPPORTED, EMPTY and sig_len rules
 * and the PSS rules are the generic path's -- and only the exponentiation between
 * them differs. Every row's status and verdict bit equal the unrouted call's under
 * both flags values; no row of these calls ever answers
 * CORDAHIP_VERIFY_UNKNOWN_KEY. cordahip_rsa_public_op_device is not routed, and
 * the K18 calls that take ids are untouched.
 * Per launch (at most the RSA workspace's rows) the route pass writes each row's key
 * id and compacts the rows that need an exponentiation into a keyed and a generic
 * list; K18's kernel runs over the keyed list and K8's over the generic list, so a
 * keyed wave holds keyed rows only. All of it runs on the caller's stream and the
 * host reads no count back. It needs 64 bytes and 12 bytes per row of the largest
 * launch of scratch beside the RSA workspace, counted in cordahip_device_mem and
 * released by cordahip_trim and the idle release with the workspace, and 16 bytes of
 * counters per device, which are kept. A batch whose scratch does not fit in device
 * memory is verified unrouted, not failed, as is a launch enqueued after the
 * device's last RSA key was removed.
 *
 * Ordering: a routed launch is a keyed call. cordahip_vkey_remove waits for the
 * routed launches already enqueued before it clears a record, so no record dies
 * between a row's match and its exponentiation; an add or a remove that races a
 * batch decides only which kernel a row takes, never its status.
 *
 * cordahip_vkey_route_stats_rsa: the rows that routed RSA enqueues on `device` have
 * matched to a registered key and not matched since cordahip_init, whether the prep
 * decided the row or not: keyed + generic is the number of rows enqueued while RSA
 * routing was on and the device held a live RSA key. The call waits for the routed
 * work already enqueued on the device. A device the context does not have, or a NULL
 * pointer, is CORDAHIP_ERR_INVALID_ARG.
 *
 * CORDAHIP_RSA_WS_ROWS (environment, tests): a multiple of 64, at least 64, caps the
 * rows of the RSA workspace and of a launch, so that the launch loop runs with a few
 * hundred rows. Unset, nothing changes. */
int cordahip_vkey_set_routing_rsa(cordahip_ctx* ctx, uint32_t on);
int cordahip_vkey_route_stats_rsa(cordahip_ctx* ctx, int device, uint64_t* keyed_rows, uint64_t* generic_rows);

/* ---- Routing inside the mixed device-resident calls (K24) ---------------------
 * cordahip_sig_verify_device, cordahip_signed_tx_verify_device and
 * cordahip_signed_txcomp_verify_device classify and pack their lanes on the GPU; only
 * the device knows how many rows each family got. K24 gives the three route passes
 * (K14, K15, K20) instances that read that count from device memory, clip it to the
 * bound the launch was sized for and partition the rows below it.
 *
 * cordahip_vkey_set_routing_device(ctx, on): on != 0 lets the three mixed device calls
 * consult the family switches on every device of the context; 0 (the default) off. It
 * takes effect with the next enqueue. Off, the three calls do exactly what they did
 * before this switch existed: nothing more is launched, allocated or locked (one
 * relaxed atomic load decides) and no route counter moves. On, each family's packed
 * rows follow that family's own switch -- cordahip_vkey_set_routing (Ed25519),
 * cordahip_vkey_set_routing_ecdsa, cordahip_vkey_set_routing_rsa -- and its own live
 * keys, by the rules stated at those switches: Ed25519 rows below the count are split
 * between K12 and K1, ECDSA rows between K13 (one run per live curve) and K2, the rows
 * of each launch of an RSA width class between K18's and K8's exponentiation. A
 * family with its switch off, with no live key or whose scratch does not fit in device
 * memory takes the unrouted launches; no batch fails because it could not be routed.
 * Every lane's status and verdict bit equal the unrouted call's under both flags
 * values. The scratch is the family's own (the dense calls' slot 0 and the RSA
 * workspace's), counted in cordahip_device_mem and released by cordahip_trim.
 *
 * Ordering: a routed mixed batch is a keyed call; cordahip_vkey_remove waits for the
 * batches already enqueued before it clears a record.
 * Counters: cordahip_vkey_route_stats, _ecdsa and _rsa also count the rows the mixed
 * calls routed, by match, with the meaning they have for the dense calls: the rows
 * below each family's count, RSA whether the prep decided the row or not.
 * A NULL context is CORDAHIP_ERR_INVALID_ARG. */
int cordahip_vkey_set_routing_device(cordahip_ctx* ctx, uint32_t on);

/* ---- RSA_SHA256 lanes in the signed-transaction host calls -------------------
 * cordahip_set_rsa_on_device(ctx, on): the context-level counterpart of
 * CORDAHIP_FLAG_RSA_ON_DEVICE for the entry points whose structs carry no flags:
 * cordahip_signed_tx_verify, cordahip_tx_submit, their _covered forms and the four
 * txcomp forms. 0 (the default): an RSA_SHA256 signature of a transaction is
 * CORDAHIP_STATUS_UNSUPPORTED there, exactly as before this switch existed. on != 0:
 * it gets exactly the status cordahip_sig_verify with CORDAHIP_FLAG_RSA_ON_DEVICE
 * and flags 0 (doVerify rules, as checkSignaturesAreValid uses) gives for the same
 * key and signature with the transaction's id as message; first_bad_sig and
 * tx_status follow from it, and a transaction whose id threw still answers the
 * id's status on every lane. It takes effect with the next call; a NULL context is
 * CORDAHIP_ERR_INVALID_ARG. cordahip_sig_verify keeps its flag and is not changed.
 * A chunk's RSA lanes are a third section of that chunk: classified and packed
 * with it by width class, their messages gathered from the ids in HBM, verified
 * on the device's RSA stream after the chunk's Ed25519 and ECDSA work and waited
 * for before the chunk's transactions are reduced. They go through the generic RSA
 * enqueue, so cordahip_vkey_set_routing_rsa applies to them.
 * Not covered: cordahip_stream_verify (its struct has no RSA section; adding one is
 * an ABI change) and the two Ed25519-only device-resident signed-tx calls. */
int cordahip_set_rsa_on_device(cordahip_ctx* ctx, uint32_t on);

/* ECDSA keygen + sign (device memory), corpus generation: per lane scheme 2/3,
 * d = SHA-256(seed) mod n, k = SHA-256(seed || msg[:64]) mod n; writes the
 * uncompressed SEC1 key (65-byte slot, key_len = 65) and the DER signature
 * (72-byte slot + sig_len). Not a production signer (deterministic synthetic nonce). */
int cordahip_ecdsa_sign_device(cordahip_ctx* ctx, int device, const void* d_scheme, const void* d_seeds,
                               const void* d_msgs, uint32_t msg_len, uint64_t n, void* d_keys, void* d_key_len,
                               void* d_sigs, void* d_sig_len, void* hip_stream);

/* ---- transaction ids and SignedTransaction batches ----------------------- */
/* tx-level statuses (tx_status[t]) in addition to the lane statuses above */
#define CORDAHIP_TX_NO_LEAVES 6     /* MerkleTreeException: empty component list (MerkleTree.kt:49-50) */
#define CORDAHIP_TX_NO_SIGNATURES 7 /* IllegalArgumentException: require(sigs.isNotEmpty()) (SignedTransaction.kt:37-39) */

/* Leaves are the serialised components of each WireTransaction, in
 * availableComponents order (MerkleTransaction.kt:51-62), each including the
 * "corda\0\0\1" Kryo header (Kryo.kt:101); the host serialises, the GPU hashes. */
typedef struct {
  uint64_t ntx;
  const uint8_t* leaf_bytes;
  const uint64_t* leaf_off;    /* [nleaves+1] into leaf_bytes */
  const uint64_t* tx_leaf_off; /* [ntx+1] leaves of tx t: [tx_leaf_off[t], tx_leaf_off[t+1]) */
  uint8_t* txid;               /* [ntx*32] out: WireTransaction.id (SecureHash bytes) */
  uint8_t* tx_status;          /* [ntx] out: OK, NO_LEAVES (ids) / first failing lane status (signed tx) */
  uint64_t nleaves;            /* ABI 4: leaves (leaf_off has nleaves+1 entries); tx_leaf_off[ntx] <= nleaves */
  uint64_t leaf_bytes_len;     /* bytes at leaf_bytes */
} cordahip_txid_batch;
int cordahip_tx_ids(cordahip_ctx* ctx, const cordahip_txid_batch* batch);

/* SignedTransaction.checkSignaturesAreValid over many transactions: every
 * signature is verified over its transaction's recomputed id; first_bad_sig[t]
 * is the index (within tx t, list order) of the signature whose exception the
 * reference would throw first, -1 if none. Signer coverage
 * (getMissingSignatures, CompositeKey.isFulfilledBy): the _covered forms and
 * cordahip_tx_cover_device below ("required-signer coverage"). */
typedef struct {
  cordahip_txid_batch tx;
  const uint64_t* tx_sig_off; /* [ntx+1] signatures of tx t */
  const uint8_t* scheme;      /* [nsig] per signature, CSR key/sig as in cordahip_sig_batch */
  const uint8_t* key;
  const uint64_t* key_off;
  const uint8_t* sig;
  const uint64_t* sig_off;
  uint8_t* sig_status;    /* [nsig] out */
  int64_t* first_bad_sig; /* [ntx] out */
  uint64_t nsig;          /* ABI 4: signatures (key_off / sig_off have nsig+1 entries); tx_sig_off[ntx] <= nsig */
  uint64_t key_bytes;     /* bytes at key */
  uint64_t sig_bytes;     /* bytes at sig */
} cordahip_signed_tx_batch;
int cordahip_signed_tx_verify(cordahip_ctx* ctx, const cordahip_signed_tx_batch* batch);

/* Ticketed forms of cordahip_signed_tx_verify / cordahip_tx_ids (SURVEY §8b
 * cordahip_tx_submit): same results, completed through cordahip_wait/poll. */
int cordahip_tx_submit(cordahip_ctx* ctx, const cordahip_signed_tx_batch* batch, uint64_t* ticket);
int cordahip_txid_submit(cordahip_ctx* ctx, const cordahip_txid_batch* batch, uint64_t* ticket);

/* Device-resident dense variant (all Ed25519, 32-byte keys, 64-byte sigs;
 * every array in HBM on `device`): K3 leaf hashes -> K4 Merkle roots ->
 * txid gather -> K1 verify -> K5 per-tx reduce, all on hip_stream. */
int cordahip_signed_tx_verify_ed25519_device(cordahip_ctx* ctx, int device, const void* d_leaf_bytes,
                                             const void* d_leaf_off, uint64_t nleaves, const void* d_tx_leaf_off,
                                             uint64_t ntx, const void* d_tx_sig_off, const void* d_keys,
                                             const void* d_sigs, uint64_t nsig, void* d_txid, void* d_tx_status,
                                             void* d_first_bad, void* d_sig_status, void* hip_stream);

/* The same for signatures of any scheme (K23): d_keys / d_sigs become a scheme byte per
 * signature and CSR keys and signatures in HBM (as cordahip_sig_verify_device takes them;
 * key_bytes / sig_bytes the byte buffers' declared sizes). The id chain is unchanged.
 * The signatures are classified and packed on the GPU, a signature's message row being
 * its transaction's id (expanded from d_tx_sig_off on the device, the ids are not copied
 * per signature), and verified by doVerify rules with the generic verifiers -- RSA_SHA256
 * on the GPU while cordahip_set_rsa_on_device is on, UNSUPPORTED otherwise, as in
 * cordahip_signed_tx_verify; registered keys are not consulted whatever
 * cordahip_vkey_set_routing* say, unless cordahip_vkey_set_routing_device is on. Then
 * K5's reduce as above: the signatures of a
 * transaction whose id failed carry that status. A signature whose ranges are out of
 * bounds is CORDAHIP_STATUS_BAD_RANGE. The _ed25519_device call stays the fast path for a
 * caller who knows the batch is dense Ed25519. */
int cordahip_signed_tx_verify_device(cordahip_ctx* ctx, int device, const void* d_leaf_bytes, const void* d_leaf_off,
                                     uint64_t nleaves, const void* d_tx_leaf_off, uint64_t ntx,
                                     const void* d_tx_sig_off, const void* d_scheme, const void* d_key,
                                     const void* d_key_off, uint64_t key_bytes, const void* d_sig,
                                     const void* d_sig_off, uint64_t sig_bytes, uint64_t nsig, void* d_txid,
                                     void* d_tx_status, void* d_first_bad, void* d_sig_status, void* hip_stream);

/* FilteredTransaction.verify over many filtered transactions:
 *   FilteredTransaction.verify   core/.../transactions/MerkleTransaction.kt:134-140
 *   PartialMerkleTree.verify     core/.../crypto/PartialMerkleTree.kt:132-158
 * Per filtered tx t: the FilteredLeaves' serialised components (leaf CSR exactly
 * as in cordahip_txid_batch; the GPU hashes them = availableComponentHashes),
 * the PartialMerkleTree as its post-order token stream tok[k] (0 IncludedLeaf,
 * 1 Leaf, 2 Node) with tok_hash[k*32 .. k*32+32) the hash of token k (ignored
 * for Node), and the claimed rootHash. tx_status[t]: OK (verify() == true),
 * BAD_SIG (verify() == false), CORDAHIP_TX_NO_LEAVES (MerkleTreeException,
 * no included leaves), CORDAHIP_TX_BAD_TREE (the token stream is not a tree:
 * no PartialMerkleTree serialises to it). */
#define CORDAHIP_TX_BAD_TREE 8
typedef struct {
  uint64_t ntx;
  const uint8_t* leaf_bytes;
  const uint64_t* leaf_off;    /* [nleaves+1] */
  const uint64_t* tx_leaf_off; /* [ntx+1] */
  const uint8_t* tok;          /* [ntok] */
  const uint8_t* tok_hash;     /* [ntok*32] */
  const uint64_t* tx_tok_off;  /* [ntx+1] */
  const uint8_t* root;         /* [ntx*32] claimed Merkle roots (FilteredTransaction.rootHash) */
  uint8_t* tx_status;          /* [ntx] out */
  uint64_t nleaves;            /* ABI 4: leaves (leaf_off has nleaves+1 entries) */
  uint64_t leaf_bytes_len;     /* bytes at leaf_bytes */
  uint64_t ntok;               /* tokens at tok (and 32-byte hashes at tok_hash) */
} cordahip_filtered_tx_batch;
int cordahip_filtered_tx_verify(cordahip_ctx* ctx, const cordahip_filtered_tx_batch* batch);
int cordahip_filtered_tx_submit(cordahip_ctx* ctx, const cordahip_filtered_tx_batch* batch, uint64_t* ticket);

/* FilteredTransaction build, the sender's side of a tear-off (what NotaryFlow.Client
 * and RatesFixFlow run before they send to a non-validating notary or an oracle):
 *   WireTransaction.buildFilteredTransaction -> FilteredTransaction.buildMerkleTransaction
 *                                core/.../transactions/MerkleTransaction.kt:121-128
 *   MerkleTree.getMerkleTree     core/.../crypto/MerkleTree.kt:27-66
 *   PartialMerkleTree.build      core/.../crypto/PartialMerkleTree.kt:68-125
 * Per transaction t: its m leaves (leaf CSR exactly as in cordahip_txid_batch)
 * and one include byte per leaf (nonzero: the JVM's filter predicate selected
 * that component; evaluating the predicate stays with the JVM). With h_i the
 * SHA-256 of leaf i and pad(m) the next power of two >= m:
 *   - membership is by hash, as the reference tests `root.hash in includeHashes`:
 *     leaf i becomes an IncludedLeaf iff some flagged leaf j has h_j == h_i,
 *     whether or not i itself is flagged;
 *   - if the number of IncludedLeafs differs from the number of flagged leaves
 *     (includeHashes.size != usedHashes.size, :75-76) the transaction fails with
 *     CORDAHIP_TX_HASHES_NOT_IN_TREE (leaves a,a,a with only the first flagged;
 *     all three flagged is OK);
 *   - a subtree with no included leaf below it is one Leaf(its hash); padding
 *     positions are Leaf(zeroHash) unless cut higher;
 *   - no flagged leaf: the single token Leaf(rootHash), status OK (the later
 *     verify() is what throws); m == 1: one token, IncludedLeaf or Leaf;
 *   - m == 0: CORDAHIP_TX_NO_LEAVES, no token, the id as cordahip_tx_ids writes it.
 * The reference's require(zeroHash !in includeHashes) (:71) cannot be reached
 * from leaf bytes -- it needs a SHA-256 preimage of 32 zero bytes -- so it has
 * no status here. Listing a hash more often than the tree holds it
 * (PartialMerkleTreeTest.kt:161-165) cannot be expressed by a mask over the
 * transaction's own leaves, and buildMerkleTransaction cannot produce it either.
 *
 * Output: txid[t] = rootHash (for every m > 0, whatever the status); the
 * post-order token stream in exactly the encoding cordahip_filtered_tx_verify
 * reads (0 IncludedLeaf, 1 Leaf, 2 Node; tok_hash of a Node is unspecified);
 * tx_ntok[t] tokens (0 for a non-OK transaction); tx_status[t].
 * Token slots are sized by the CALLER: tx_tok_off is an input, transaction t
 * owns entries [tx_tok_off[t], tx_tok_off[t+1]) of tok and tok_hash and its
 * tokens are written from the slot's start. A slot must hold 2*pad(m) - 1
 * tokens (0 for m == 0), the exact worst case. Slot entries at or past
 * tx_ntok[t] are unspecified; nothing outside [tx_tok_off[0], tx_tok_off[ntx])
 * is written. The host forms check every slot (and the CSR levels) before any
 * enqueue: a violation is CORDAHIP_ERR_INVALID_ARG with the outputs untouched. */
#define CORDAHIP_TX_HASHES_NOT_IN_TREE 12 /* MerkleTreeException, PartialMerkleTree.kt:75-76 */
#define CORDAHIP_TX_TOK_SLOT_TOO_SMALL 13 /* device-resident call only: slot < 2*pad(m)-1 */
typedef struct {
  uint64_t ntx;
  const uint8_t* leaf_bytes;
  const uint64_t* leaf_off;    /* [nleaves+1] into leaf_bytes */
  const uint64_t* tx_leaf_off; /* [ntx+1] */
  const uint8_t* include;      /* [nleaves] nonzero: the filter selected this component */
  const uint64_t* tx_tok_off;  /* [ntx+1] in: token slots */
  uint8_t* txid;               /* [ntx*32] out: rootHash */
  uint8_t* tok;                /* [ntok] out */
  uint8_t* tok_hash;           /* [ntok*32] out */
  uint64_t* tx_ntok;           /* [ntx] out */
  uint8_t* tx_status;          /* [ntx] out */
  uint64_t nleaves;            /* leaves (leaf_off has nleaves+1 entries, include nleaves) */
  uint64_t leaf_bytes_len;     /* bytes at leaf_bytes */
  uint64_t ntok;               /* token entries at tok (and 32-byte hashes at tok_hash) */
} cordahip_filtered_build_batch;
int cordahip_filtered_tx_build(cordahip_ctx* ctx, const cordahip_filtered_build_batch* batch);
int cordahip_filtered_tx_build_submit(cordahip_ctx* ctx, const cordahip_filtered_build_batch* batch,
                                      uint64_t* ticket);
/* Device-resident form: every array in HBM on `device`, K3 and K10 on
 * hip_stream. Its offsets are read on the device only, so the kernel guards
 * the slots itself: a transaction whose slot is smaller than 2*pad(m) - 1 (or
 * reversed, or reaching past ntok) gets CORDAHIP_TX_TOK_SLOT_TOO_SMALL, its
 * id, tx_ntok[t] = 0 and no token; a failed count rule is reported first. The
 * leaf-level offsets are the caller's contract, as in
 * cordahip_signed_tx_verify_ed25519_device. */
int cordahip_filtered_tx_build_device(cordahip_ctx* ctx, int device, const void* d_leaf_bytes,
                                      const void* d_leaf_off, uint64_t nleaves, const void* d_tx_leaf_off,
                                      uint64_t ntx, const void* d_include, const void* d_tx_tok_off, uint64_t ntok,
                                      void* d_txid, void* d_tok, void* d_tok_hash, void* d_tx_ntok,
                                      void* d_tx_status, void* hip_stream);

/* ---- native Kryo leaf encoder ------------------------- *
 * The Merkle leaf of a transaction component is SHA-256 of its p2p Kryo bytes:
 *   serializedHash(x) = p2PKryo().withoutReferences { x.serialize(kryo).hash }
 *       core/.../transactions/MerkleTransaction.kt:16-18
 *   serialize = "corda\0\0\1" header + kryo.writeClassAndObject(x)
 *       core/.../serialization/Kryo.kt:101,165-176
 * cordahip_kryo_encode writes those preimages natively (no JVM re-serialisation)
 * for the component kinds whose wire form is fixed by Kryo 4.0.0's published
 * format plus Corda's own serializers; any other component travels as a RAW,
 * already-serialised leaf. Output is the leaf CSR cordahip_tx_ids consumes.
 * Kinds and their bytes after the header (varint = Kryo writeVarInt(x, true)):
 *   RAW            data[len] copied verbatim (a complete leaf, header included)
 *   CHAR/SHORT/INT/LONG/BYTE/BOOLEAN/FLOAT/DOUBLE  (boxed primitive, Kryo's
 *                  default registrations 5/6/0/7/4/3/2/8): varint(id + 2), then
 *                  the value big-endian in 2/2/4/8/1/1/4/8 bytes (value: bits)
 *   STRING         varint(1 + 2), Output.writeString of the UTF-16 code units
 *                  data[0..2*len) (little-endian u16): ASCII form for 2..63 ASCII
 *                  chars, else UTF-8 length + modified UTF-8
 *   ED25519_KEY    varint(class_id + 2), varint(32), A (Ed25519PublicKeySerializer,
 *                  Kryo.kt:383-393); data = the 32-byte A
 *   PUBLIC_KEY     varint(class_id + 2), varint(len), key.encoded (PublicKeySerializer,
 *                  Kryo.kt:441-451, BCEC/BCRSA/SPHINCS keys); data = X.509 SPKI DER
 *   KOTLIN_OBJECT  varint(NAME + 2 = 1), varint(name id 0), writeString(class
 *                  name) and no body (CordaClassResolver.registerImplicit's
 *                  KotlinObjectSerializer, CordaClassResolver.kt:76-99), e.g.
 *                  "net.corda.core.contracts.TransactionType$General"; data =
 *                  the class name as UTF-16 code units (len = chars)
 *   PARTY          the notary Party (identity/Party.kt): NAME registration of
 *                  "net.corda.core.identity.Party", CompatibleFieldSerializer
 *                  (EXTENDED names, DefaultKryoCustomizer.kt:56-58) over
 *                  AbstractParty.owningKey (key class + writeBytesWithLength) and
 *                  Party.name (X500NameSerializer, Kryo.kt:615-624); data = the
 *                  X.500 name's DER (self-delimiting) followed by the key bytes
 *                  (A, or the SPKI DER); class_id = X500Name's registration id;
 *                  value = the key class's registration id
 *   ISSUE_COMMAND  Command(value = an issue command data class with one Long
 *                  `nonce`, signers = Arrays.asList(keys)) as
 *                  TransactionBuilder.addCommand(data, vararg keys) builds it
 *                  (TransactionBuilder.kt:124, Structures.kt:285, Cash.kt:148);
 *                  data = u8 class-name length, the command data's binary class
 *                  name, u8 key count, per key u16 LE registration id, u16 LE
 *                  length, key bytes; class_id = java.util.Arrays$ArrayList's
 *                  registration id (ArraysAsListSerializer); value = the nonce
 *   CASH_STATE     TransactionState<Cash.State> -- the output of a cash issue
 *                  (Cash.generateIssue, Cash.kt:166-167; Structures.kt:95-117,
 *                  132,268; Cash.kt:35,62,92-103; Amount.kt:37): TransactionState
 *                  (data, encumbrance, notary) > Cash.State (amount, contract =
 *                  CASH_PROGRAM_ID, exitKeys = {owner key, issuer key},
 *                  owner, participants = [owner]) > Amount(quantity,
 *                  displayTokenSize = 10^-digits, Issued(PartyAndReference(
 *                  issuer, reference), Currency)). data = issuer party, u8
 *                  reference length, reference bytes, owner party, notary party,
 *                  u8 currency-code length, the code (ASCII), i8 the currency's
 *                  fraction digits, the 32-byte legalContractReference
 *                  (SHA-256 of Cash's legal-prose URL), u8 flags (bit 0:
 *                  encumbrance present), i32 LE encumbrance; a party = u16 LE key
 *                  registration id, u16 LE key length, key bytes, u16 LE X.500
 *                  name length, the name's DER (length 0 = AnonymousParty, e.g.
 *                  CashIssueFlow's anonymised recipient; the notary must be a
 *                  Party); class_id = X500Name's registration id; value = the
 *                  quantity (pennies)
 * Field values go through OutputChunked (1024-byte chunks + a zero chunk) as
 * Kryo 4.0.0's CompatibleFieldSerializer writes them, nested serializers'
 * flushes cutting the enclosing fields' chunks (kryo.cpp). PARTY / ISSUE_COMMAND
 * / CASH_STATE are restated from Kryo 4.0.0 / kryo-serializers 0.41 published
 * sources: PARITY
 * UNPINNED (no JVM here), except the Ed25519 key bytes inside them, which the
 * reference's own serialised keys pin (tests/golden/kryo_key_vectors.json).
 * class_id = kryo.getRegistration(cls).id on the node (registration order of
 * DefaultKryoCustomizer.kt is fixed per build; the JVM reads it once).
 * off[0..n] receives the CSR offsets; returns CORDAHIP_ERR_BUFFER_TOO_SMALL with
 * off[n] = the bytes needed when cap is too small, and CORDAHIP_ERR_INVALID_ARG
 * at the first invalid item -- `out` (and off) are then left partly written:
 * the leaves before that item are in place. Host-only: no device work. */
#define CORDAHIP_ERR_BUFFER_TOO_SMALL (-8)
#define CORDAHIP_KRYO_RAW 0
#define CORDAHIP_KRYO_CHAR 1
#define CORDAHIP_KRYO_SHORT 2
#define CORDAHIP_KRYO_INT 3
#define CORDAHIP_KRYO_LONG 4
#define CORDAHIP_KRYO_BYTE 5
#define CORDAHIP_KRYO_BOOLEAN 6
#define CORDAHIP_KRYO_FLOAT 7
#define CORDAHIP_KRYO_DOUBLE 8
#define CORDAHIP_KRYO_STRING 9
#define CORDAHIP_KRYO_ED25519_KEY 10
#define CORDAHIP_KRYO_PUBLIC_KEY 11
#define CORDAHIP_KRYO_KOTLIN_OBJECT 12
#define CORDAHIP_KRYO_PARTY 13
#define CORDAHIP_KRYO_ISSUE_COMMAND 14
#define CORDAHIP_KRYO_CASH_STATE 15
/* The two components a non-validating notary is shown (NotaryFlow.kt:62 reveals
 * `it is StateRef || it is TimeWindow`). Both classes are @CordaSerializable and
 * unregistered: NAME registration, CompatibleFieldSerializer with EXTENDED names.
 *   STATE_REF      net.corda.core.contracts.StateRef(txhash, index)
 *                  (Structures.kt:247). Fields in name order: StateRef.index, a
 *                  primitive int: Output.writeInt(v, false), the zig-zag varint;
 *                  StateRef.txhash, declared SecureHash (not final): the class
 *                  net.corda.core.crypto.SecureHash$SHA256 by name, then its one
 *                  field OpaqueBytes.bytes (varint(33), the 32 bytes). data = one
 *                  cordahip_state_ref row (32 bytes txhash, u32 LE index read as a
 *                  Java int), len = 36; class_id and value unused. 173..177 bytes.
 *   TIME_WINDOW    net.corda.core.contracts.TimeWindow(fromTime, untilTime)
 *                  (Structures.kt:336-341), two nullable java.time.Instant fields
 *                  TimeWindow.fromTime, TimeWindow.untilTime. Instant is final, so
 *                  no class is written: a side is NULL (00) or NOT_NULL (01) and the
 *                  Instant body. THE BODY IS TAKEN TO BE Kryo 4.0.0's
 *                  TimeSerializers.InstantSerializer: writeLong(epochSecond, true),
 *                  writeInt(nano, true) -- plain varints, a negative second takes 9
 *                  bytes. That TimeSerializers is among Kryo 4.0.0's default
 *                  serializers is recalled from its published source, not checked
 *                  against it here (no Kryo source, no JVM). data, len = 25: u8
 *                  flags (bit 0 fromTime present, bit 1 untilTime present), i64 LE
 *                  from-epochSecond, i32 LE from-nano, i64 LE until-epochSecond, i32
 *                  LE until-nano. Invalid: another len, flags & ~3, a present side
 *                  with nano outside [0, 999999999] or seconds outside Instant's
 *                  range [-31557014167219200, 31556889864403199]. flags == 0 is
 *                  encoded (two NULL markers). 91..119 bytes.
 * Both are PARITY UNPINNED like PARTY / ISSUE_COMMAND / CASH_STATE; the vectors
 * in tests/golden/notary_leaf_vectors.json are derived from the same published
 * rules by the test model, not taken from a JVM. */
#define CORDAHIP_KRYO_STATE_REF 16
#define CORDAHIP_KRYO_TIME_WINDOW 17
/* What a payment adds to a cash issue's components (K22): its command, and an
 * attachment id.
 *   MOVE_COMMAND   net.corda.core.contracts.Command(value, signers)
 *                  (Structures.kt:285) whose value is a Move data class with the one
 *                  field contractHash: SecureHash? (Cash.kt:142,
 *                  CommodityContract.kt:125, Obligation.kt:348,
 *                  CommercialPaper.kt:190). Command and the Move class by NAME, each
 *                  through CompatibleFieldSerializer, as ISSUE_COMMAND; the Move
 *                  class's field is "<Simple>.contractHash", <Simple> the class name
 *                  after its last '$' or '.'. The field is declared SecureHash? and not
 *                  final: null is writeClass(null), one byte 00; a hash is the class
 *                  net.corda.core.crypto.SecureHash$SHA256 by NAME and then
 *                  OpaqueBytes.bytes, as STATE_REF's txhash. Command.signers comes in
 *                  two list forms: TransactionBuilder.addCommand(data, vararg keys)
 *                  gives java.util.Arrays$ArrayList (ArraysAsListSerializer, as
 *                  ISSUE_COMMAND: class_id, length, component class
 *                  java.security.PublicKey by NAME, the elements);
 *                  OnLedgerAsset.generateSpend (OnLedgerAsset.kt:93,121) passes
 *                  gathered.map { }, a java.util.ArrayList, which is unregistered
 *                  (DefaultKryoCustomizer.kt): by NAME through Kryo's
 *                  CollectionSerializer, varint(size) then class and object per
 *                  element, as CASH_STATE's exitKeys. data = ISSUE_COMMAND's layout
 *                  (u8 name length, the binary class name, u8 key count, per key u16 LE
 *                  registration id, u16 LE length, key bytes), then u8 flags (bit 0:
 *                  contractHash present, bit 1: the signers are a java.util.ArrayList,
 *                  else Arrays$ArrayList), then the 32 hash bytes iff bit 0. class_id =
 *                  Arrays$ArrayList's registration id, ignored with bit 1; value
 *                  unused. Invalid: name length < 2, no key, a zero-length key,
 *                  flags & ~3, a payload that does not end where the layout ends. With
 *                  one to three Ed25519 signers a Cash move is 199 / 233 / 267 bytes
 *                  (java.util.ArrayList, no hash) up to 300 / 334 / 369
 *                  (Arrays$ArrayList, with the hash): 4 to 6 SHA-256 blocks (the table
 *                  is in DESIGN §4 K22). Cash.Commands.Exit and the non-cash commands
 *                  are not covered.
 *   SECURE_HASH    an attachment id as a component (WireTransaction.attachments:
 *                  List<SecureHash>): SecureHash$SHA256 by NAME (name id 0), then
 *                  OpaqueBytes.bytes. data = the 32 bytes, len = 32, anything else is
 *                  invalid; class_id and value unused. 102 bytes.
 * Both are PARITY UNPINNED like every composite kind above; the vectors in
 * tests/golden/payment_leaf_vectors.json are derived from the same published rules
 * by the test model (tests/kryo_payment_model.py), not taken from a JVM. */
#define CORDAHIP_KRYO_MOVE_COMMAND 18
#define CORDAHIP_KRYO_SECURE_HASH 19
typedef struct {
  uint32_t kind;       /* CORDAHIP_KRYO_* */
  uint32_t class_id;   /* Kryo registration id (ED25519_KEY, PUBLIC_KEY) */
  int64_t value;       /* primitive kinds: the value (FLOAT / DOUBLE: the IEEE bits) */
  const uint8_t* data; /* RAW / STRING / key / class-name payload */
  uint64_t len;        /* bytes (RAW, keys) or UTF-16 code units (STRING, KOTLIN_OBJECT) */
} cordahip_kryo_item;
int cordahip_kryo_encode(const cordahip_kryo_item* items, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* off);

/* The same leaf preimages computed on the GPU, for components whose payloads
 * are already in device memory (a transaction batch's ids then need neither
 * host serialisation nor leaf bytes over PCIe). d_items: n items in device
 * memory whose `data` are device pointers; group: the items come as records of
 * `group` components (e.g. the 5 of a cash-issue transaction) -- a thread
 * mapping hint, 1 = none. Writes d_off[0..n] (uint64, the CSR offsets; d_off[n]
 * = the bytes of all leaves) and d_status[i] (uint8): 0 written, 1 invalid item
 * (as cordahip_kryo_encode would reject it; size 0), 2 not written because it
 * ends beyond cap. Enqueued on hip_stream, asynchronous; the caller reads
 * d_off[n] / d_status when it needs them. Same encoder as cordahip_kryo_encode
 * (corda_amd/csrc/kryo_core.hpp): bit-identical leaves; items of one shape
 * (equal structure, kryo_template.hpp) are written from a template traced once
 * per shape. d_out NULL: sizes and offsets only (statuses 0 / 1). n < 2^31 - 1
 * per call. Device scratch (grow-only, per device): 16 B per item, ~18 MB of
 * shape table and templates, 56 MB of level buffers for the items written
 * without a template. */
int cordahip_kryo_encode_device(cordahip_ctx* ctx, int device, const void* d_items, uint64_t n, uint32_t group,
                                void* d_out, uint64_t cap, void* d_off, void* d_status, void* hip_stream);

/* ---- component-level SignedTransaction batches (SURVEY §8b + §8f rank 4) ---- *
 * cordahip_signed_tx_verify with each transaction's COMPONENTS instead of their
 * serialised leaves: the JVM hands over the Kryo items of availableComponents
 * (MerkleTransaction.kt:51-62) and the GPU writes the leaf preimages
 * (serializedHash, MerkleTransaction.kt:16-18; the encoder of
 * cordahip_kryo_encode_device) ahead of K3 / K4, so tx ids need no JVM
 * re-serialisation and PCIe carries the components (~540 B per cash-issue
 * transaction: 160 B of items, 379 B of payload) instead of the leaves
 * (1,717 B). Once a device's component batches need no new template and no
 * direct encoder, it runs a templates-only encoder chain; a call that then
 * meets a new shape runs again with the full chain before it returns (same
 * outputs, about twice the time for that call). Replaces the same reference
 * calls as cordahip_tx_submit: SignedTransaction.checkSignaturesAreValid
 * (SignedTransaction.kt:95-100) + the id of verifySignatures (:70-85,
 * WireTransaction.kt:48).
 * items[i].data is an OFFSET into `payload` (not a pointer); any number of
 * items may share a payload (the notary Party, TransactionType). The payload
 * crosses PCIe as a growing prefix, slice by slice: laid out in transaction
 * order (shared payloads first) the first slice's copy stays short. An item
 * whose payload runs past payload_len, or that cordahip_kryo_encode would
 * reject, makes its transaction CORDAHIP_TX_BAD_COMPONENT (its id is not
 * computed; serialise that transaction on the JVM and use RAW leaves).
 * Signature fields, outputs and statuses as in cordahip_signed_tx_batch.     */
#define CORDAHIP_TX_BAD_COMPONENT 9
typedef struct {
  uint64_t ntx;
  const cordahip_kryo_item* items; /* [nitems] components, tx by tx, availableComponents order */
  const uint64_t* tx_item_off;     /* [ntx+1] items of tx t: [tx_item_off[t], tx_item_off[t+1]) */
  const uint8_t* payload;          /* item payloads (data = offsets into it) */
  uint64_t payload_len;
  uint8_t* txid;      /* [ntx*32] out */
  uint8_t* tx_status; /* [ntx] out */
  uint64_t n_items;   /* ABI 4: records at items; tx_item_off[ntx] <= n_items */
} cordahip_txcomp_batch;
typedef struct {
  cordahip_txcomp_batch tx;
  const uint64_t* tx_sig_off; /* [ntx+1] */
  const uint8_t* scheme;      /* [nsig] */
  const uint8_t* key;
  const uint64_t* key_off;
  const uint8_t* sig;
  const uint64_t* sig_off;
  uint8_t* sig_status;    /* [nsig] out */
  int64_t* first_bad_sig; /* [ntx] out */
  uint64_t nsig;          /* ABI 4: signatures (key_off / sig_off have nsig+1 entries) */
  uint64_t key_bytes;     /* bytes at key */
  uint64_t sig_bytes;     /* bytes at sig */
} cordahip_signed_txcomp_batch;
int cordahip_signed_txcomp_verify(cordahip_ctx* ctx, const cordahip_signed_txcomp_batch* batch);
int cordahip_txcomp_submit(cordahip_ctx* ctx, const cordahip_signed_txcomp_batch* batch, uint64_t* ticket);

/* Device-resident component-level variant (all Ed25519, 32-byte keys, 64-byte
 * sigs; every array in HBM on `device`, items[i].data OFFSETS into d_payload as
 * in cordahip_txcomp_batch): the components' leaf hashes straight from the
 * encoder's per-shape templates (no leaf bytes; new shapes are traced in the
 * same launch set, items without a template go through the direct encoder into
 * a SHA-256 sink, so there is no miss and no second pass) -> K4 Merkle roots ->
 * txid gather -> K1 verify -> K5 per-tx reduce, all on hip_stream. The ids of
 * cordahip_signed_txcomp_verify / cordahip_signed_tx_verify over the same
 * components' leaves; a rejected component makes its transaction
 * CORDAHIP_TX_BAD_COMPONENT and its signatures carry that status (as a failed
 * id does in every signed-tx path). group: as in cordahip_kryo_encode_device.
 * d_tx_item_off / d_tx_sig_off [ntx+1] (uint64) index d_items / the signatures
 * from 0; device memory is the caller's contract (not readable from the host).
 * n_items < 2^31 - 1. Replaces the same reference calls as
 * cordahip_txcomp_submit (SignedTransaction.kt:95-100, WireTransaction.kt:48,
 * MerkleTransaction.kt:16-18). */
int cordahip_signed_txcomp_verify_ed25519_device(cordahip_ctx* ctx, int device, const void* d_items,
                                                 uint64_t n_items, uint32_t group, const void* d_payload,
                                                 uint64_t payload_len, const void* d_tx_item_off, uint64_t ntx,
                                                 const void* d_tx_sig_off, const void* d_keys, const void* d_sigs,
                                                 uint64_t nsig, void* d_txid, void* d_tx_status, void* d_first_bad,
                                                 void* d_sig_status, void* hip_stream);
/* ... and for signatures of any scheme (K23): the component-level call with the
 * signatures as cordahip_signed_tx_verify_device takes them, and its rules. */
int cordahip_signed_txcomp_verify_device(cordahip_ctx* ctx, int device, const void* d_items, uint64_t n_items,
                                         uint32_t group, const void* d_payload, uint64_t payload_len,
                                         const void* d_tx_item_off, uint64_t ntx, const void* d_tx_sig_off,
                                         const void* d_scheme, const void* d_key, const void* d_key_off,
                                         uint64_t key_bytes, const void* d_sig, const void* d_sig_off,
                                         uint64_t sig_bytes, uint64_t nsig, void* d_txid, void* d_tx_status,
                                         void* d_first_bad, void* d_sig_status, void* hip_stream);

/* ---- required-signer coverage (the second half of verifySignatures) ---------- *
 * SignedTransaction.verifySignatures (SignedTransaction.kt:70-85) is
 * checkSignaturesAreValid (:95-100, the calls above) and then
 *   getMissingSignatures (:102-108): tx.mustSign.filter { !it.isFulfilledBy(sigKeys) }
 *   PublicKey.isFulfilledBy          CryptoUtils.kt:79-82
 *   CompositeKey.isFulfilledBy       CompositeKey.kt:186-209 (threshold trees)
 *   missing - allowedToBeMissing, SignaturesMissingException (:76-82).
 * A cordahip_cover carries every transaction's required keys (tx.mustSign, list
 * order); the library answers per required key (req_status) and per transaction
 * (tx_status, first_missing). The .toSet() de-duplication of the missing keys
 * and getMissingKeyDescriptions (:114-124) stay with the caller: both are read
 * off req_status.
 *
 * A required key is a POST-ORDER token stream: a leaf pushes one value, a node
 * with nchild children takes the nchild values before it. A plain PublicKey is
 * one leaf token. Leaves index a key table (ckey_scheme / ckey / ckey_off) whose
 * entries any number of leaves, of any transaction, may share.
 *
 * Leaf fulfilment: a leaf is fulfilled iff some signature of the SAME
 * transaction has the same scheme byte, the same key length and the same key
 * bytes (keysToCheck.contains(node), CompositeKey.kt:192). The scheme takes part
 * in the comparison: the same 33 or 65 bytes under secp256k1 and secp256r1 are
 * different keys. The caller supplies ONE canonical encoding on both sides (the
 * signature's key and the table's): the compressed and the uncompressed SEC1
 * form of one point are equal for BCECPublicKey.equals but NOT here.
 * Node fulfilment: a node is fulfilled iff the summed weights of its fulfilled
 * children are >= threshold (checkFulfilledBy, CompositeKey.kt:186-196).
 * The root's own weight is ignored.
 *
 * A required key is CORDAHIP_REQ_MALFORMED when CompositeKey.checkValidity
 * (:110-122) would throw from checkConstraints (:73-85) / totalWeight
 * (:126-133), or when the stream is no tree:
 *   - an empty token range;
 *   - a stream that does not reduce to exactly one value;
 *   - a node with nchild == 1 (:77), or with more children than there are
 *     values before it;
 *   - a threshold of 0 (:79), or above the children's total weight (:82);
 *   - a child weight of 0 (:129); a weight or threshold above 2^31 - 1 is not a
 *     Java positive Int and counts as non-positive;
 *   - a total weight above 2^31 - 1 (Math.addExact, :130);
 *   - a leaf whose key >= nckey.
 * Duplicate children (:74) are NOT looked for: that needs structural subtree
 * equality, and the JVM's CompositeKey constructor has already enforced it.
 * Cycles cannot be expressed in a token stream.
 *
 * Per transaction, in this order:
 *   1. tx_status[t] != OK on entry (NO_SIGNATURES, NO_LEAVES, BAD_COMPONENT or
 *      any signature's status): its entries are NOT_EVALUATED, tx_status[t] is
 *      unchanged, first_missing[t] = -1.
 *   2. Otherwise every entry is evaluated on its own.
 *   3. Any MALFORMED entry: tx_status[t] = CORDAHIP_TX_BAD_COVER and
 *      first_missing[t] = the first malformed entry (filter runs to the end, so
 *      the first invalid key throws before any missing set is built).
 *   4. Otherwise any MISSING entry: CORDAHIP_TX_SIGNATURES_MISSING and
 *      first_missing[t] = the first MISSING entry; MISSING_ALLOWED entries do
 *      not count.
 *   5. Otherwise OK. A transaction without required keys is OK.
 * tx_req_off, req_tok_off and ckey_off are CSR arrays, checked as every CSR array
 * of this header is (within nreq / ntok / ckey_bytes, non-decreasing, whole,
 * before any enqueue: CORDAHIP_ERR_INVALID_ARG, the context stays usable).     */
#define CORDAHIP_TX_SIGNATURES_MISSING 10 /* SignaturesMissingException (SignedTransaction.kt:81) */
#define CORDAHIP_TX_BAD_COVER 11          /* IllegalArgumentException from CompositeKey.checkValidity (:110-122) */

/* req_status[r] */
#define CORDAHIP_REQ_FULFILLED 0
#define CORDAHIP_REQ_MISSING 1
#define CORDAHIP_REQ_MISSING_ALLOWED 2 /* missing, but the caller flagged it allowedToBeMissing */
#define CORDAHIP_REQ_NOT_EVALUATED 3   /* the tx had already failed (id or a signature) */
#define CORDAHIP_REQ_MALFORMED 4

typedef struct {      /* 16 bytes; one required key = a POST-ORDER token stream */
  uint32_t nchild;    /* 0: leaf; >= 2: CompositeKey node over the nchild subtrees before it */
  uint32_t weight;    /* this node's weight in its parent (ignored at the root) */
  uint32_t threshold; /* nodes only */
  uint32_t key;       /* leaves only: index into the cover key table */
} cordahip_cover_tok;

typedef struct {
  const uint64_t* tx_req_off;    /* [ntx+1] required keys (tx.mustSign entries, list order) of tx t */
  const uint64_t* req_tok_off;   /* [nreq+1] tokens of required key r */
  const cordahip_cover_tok* tok; /* [ntok] */
  const uint8_t* req_flags;      /* [nreq] bit 0: allowed to be missing; NULL = none */
  const uint8_t* ckey_scheme;    /* [nckey] CORDAHIP_SCHEME_* */
  const uint8_t* ckey;           /* key table, CSR; entries may be shared by any number of leaves */
  const uint64_t* ckey_off;      /* [nckey+1] */
  uint8_t* req_status;           /* [nreq] out */
  int64_t* first_missing;        /* [ntx] out: index within tx t's required keys, -1 if none */
  uint64_t nreq, ntok, nckey, ckey_bytes;
} cordahip_cover;

/* The rule alone, on the host: no context, no device work (the JVM's fallback
 * path, and what the device kernel is tested against). tx_status [ntx] in/out
 * as described above; the signature keys as in cordahip_signed_tx_batch
 * (tx_sig_off [ntx+1] within nsig, scheme [nsig], key / key_off CSR within
 * key_bytes), checked like the cover's own arrays. */
int cordahip_cover_eval_host(const cordahip_cover* cover, uint64_t ntx, uint8_t* tx_status,
                             const uint64_t* tx_sig_off, const uint8_t* scheme, const uint8_t* key,
                             const uint64_t* key_off, uint64_t nsig, uint64_t key_bytes);

/* cordahip_signed_tx_verify / cordahip_tx_submit / cordahip_signed_txcomp_verify
 * / cordahip_txcomp_submit followed by the coverage rule: the whole of
 * verifySignatures in one call. Coverage runs on the host threads next to each
 * device, over the same transaction ranges and directly after the
 * per-transaction reduce -- the signature keys and statuses are in host memory
 * there already. The ticketed forms copy the cover descriptor at submit, as
 * they copy the batch descriptor; its arrays stay the caller's until wait. */
int cordahip_signed_tx_verify_covered(cordahip_ctx* ctx, const cordahip_signed_tx_batch* batch,
                                      const cordahip_cover* cover);
int cordahip_tx_submit_covered(cordahip_ctx* ctx, const cordahip_signed_tx_batch* batch, const cordahip_cover* cover,
                               uint64_t* ticket);
int cordahip_signed_txcomp_verify_covered(cordahip_ctx* ctx, const cordahip_signed_txcomp_batch* batch,
                                          const cordahip_cover* cover);
int cordahip_txcomp_submit_covered(cordahip_ctx* ctx, const cordahip_signed_txcomp_batch* batch,
                                   const cordahip_cover* cover, uint64_t* ticket);

/* The device-resident form: `cover` is a HOST struct whose pointers are DEVICE
 * memory on `device`, d_tx_status [ntx] in/out. Stream-ordered: enqueue it on
 * the stream of cordahip_signed_tx_verify_ed25519_device /
 * cordahip_signed_txcomp_verify_ed25519_device right after that call, with the
 * same d_tx_status / d_tx_sig_off / d_keys, and the verdict of verifySignatures
 * never leaves the device. d_sig_scheme NULL: every signature is Ed25519;
 * d_sig_key_off NULL: d_sig_key holds dense 32-byte rows (16-byte aligned),
 * else CSR keys. One lane per transaction; lanes do scattered reads of their
 * keys. The offset arrays in device memory are the caller's contract, as for
 * the other device calls (an offset beyond its level's declared count makes
 * the transaction BAD_COVER rather than a read outside the arrays); token
 * contents are data and checked. Device scratch (grow-only, per device,
 * released by cordahip_trim and the idle release): 8 B per token. */
int cordahip_tx_cover_device(cordahip_ctx* ctx, int device, uint64_t ntx, void* d_tx_status,
                             const void* d_tx_sig_off, const void* d_sig_scheme, const void* d_sig_key,
                             const void* d_sig_key_off, const cordahip_cover* cover, void* hip_stream);

/* ---- notary commit log: batched uniqueness check (K16) ------------------------ *
 * The middle of NotaryFlow.Service.call (NotaryFlow.kt:98-104) for a batch:
 * service.validateTimeWindow (NotaryService.kt:44-47, TimeWindowChecker.kt:14-25)
 * and service.commitInputStates (NotaryService.kt:53-67 ->
 * PersistentUniquenessProvider.commit, PersistentUniquenessProvider.kt:62-82) over
 * a device-resident index of the consumed StateRefs and their ConsumingTx. A
 * batch gets exactly the answers the serial provider gives when it takes the
 * transactions one at a time in batch order, whatever the log held before. The
 * log is the in-memory index the provider's map is: the database stays the
 * durable record (the caller persists the rows of the transactions marked
 * `committed`), and consensus is not touched.
 *
 * Per transaction t, in batch order:
 *   gate[t] != 0                       CORDAHIP_COMMIT_SKIPPED, nothing looked up
 *   time window invalid                CORDAHIP_COMMIT_TIME_WINDOW_INVALID, nothing
 *     (until present and now - until > tolerance, or from present and
 *      from - now > tolerance; exact in ns, exactly `tolerance` is valid)
 *   no input in the log                every refs[i] -> (txid, i, caller) put in list
 *                                      order (a ref listed twice keeps its LAST
 *                                      position); OK, committed = 1; also with no inputs
 *   every present input i stores exactly (txid, i, caller)
 *                                      OK, committed = 0 (already committed: the
 *                                      notary signs again), NOTHING inserted -- not
 *                                      even inputs that were absent
 *   otherwise                          CORDAHIP_COMMIT_CONFLICT, committed = 0,
 *                                      nothing inserted
 * ref_state[i] / ref_by[i] for the three last outcomes: 0 absent (zero row), 1
 * consumed by exactly this (txid, i, caller), 2 consumed by another -- ref_by the
 * stored record; the conflict's stateHistory is every input with ref_state != 0.
 * Skipped and out-of-window transactions get zero rows.
 *
 * Chaining. OK is 0 for "committed" and "already committed" alike, so tx_status
 * goes straight in as the signer's gate (cordahip_sign's gate,
 * cordahip_ed25519_sign_keyed_device's d_gate), and `gate` takes
 * cordahip_filtered_tx_verify's tx_status. With the device form nothing is read
 * back to the host between the calls.
 * Time bounds. tw_from / tw_until that do not fit are saturated by the caller at
 * +-2^62 ns; INT64_MIN marks an absent side. |now_ns| < 2^61 and
 * 0 <= tolerance_ns < 2^61, else CORDAHIP_ERR_INVALID_ARG: no difference overflows.
 * Capacity. 2^capacity_log2 slots of 96 bytes (6 <= capacity_log2 <= 32), fixed
 * between cordahip_commit_log_reserve calls. The host keeps an upper bound of the
 * live entries: every commit call adds its n_refs and every load its n, whatever
 * the outcomes; cordahip_commit_log_stats reads the exact count back and tightens
 * the bound. A call whose bound would pass 7/8 of the capacity returns
 * CORDAHIP_ERR_LOG_FULL before any enqueue, the log and the outputs untouched.
 * Below that load linear probing always finds a slot: there is no per-transaction
 * "full" status, and the device form never reads a counter back.
 * Ordering. Calls on one log are serialised in enqueue order (a lock per log, and
 * an event fence when the caller's stream differs from the previous call's); two
 * tickets submitted one after the other from one thread commit in submit order
 * (the ticket queue of a log is drained in order). destroy and reserve wait for
 * every call already enqueued.
 * Memory and ids. The table is counted in cordahip_device_mem; cordahip_trim and
 * the idle release keep it (like the signer's table); destroy and
 * cordahip_shutdown free it. A log id is never reused.
 * Load. cordahip_commit_log_load inserts rows with sequence number 0, older than
 * every batch; a row whose ref is present already (in the log, or earlier in the
 * same call) is counted in *n_already_present and left alone.
 * Devices. A log lives on the one device named at creation.
 * The slot index is a keyed hash (SipHash-1-3) of the 36 ref bytes under the
 * log's 128-bit salt (NULL: drawn by the library): ref bytes are client-chosen.
 * CSR: tx_ref_off[0..ntx] non-decreasing and tx_ref_off[ntx] <= n_refs, checked
 * whole before any enqueue (host forms). In the device form an offset beyond
 * n_refs is cut to n_refs on the device, so no kernel indexes outside the arrays;
 * device pointers are 8-byte aligned (uint64 / int64 arrays) or 4-byte aligned. */
#define CORDAHIP_COMMIT_CONFLICT 16            /* NotaryError.Conflict (UniquenessException) */
#define CORDAHIP_COMMIT_TIME_WINDOW_INVALID 17 /* NotaryError.TimeWindowInvalid */
#define CORDAHIP_COMMIT_SKIPPED 18             /* gate[t] != 0 */
#define CORDAHIP_ERR_LOG_FULL (-9)
typedef struct { uint8_t txhash[32]; uint32_t index; } cordahip_state_ref;                       /* 36 B rows */
typedef struct { uint8_t id[32]; uint32_t input_index; uint32_t caller; } cordahip_consuming_tx; /* 40 B rows */
typedef struct { cordahip_state_ref ref; cordahip_consuming_tx by; } cordahip_commit_row;        /* 76 B rows */

int cordahip_commit_log_create(cordahip_ctx* ctx, int device, uint32_t capacity_log2, const uint8_t salt[16],
                               uint32_t* log_id);
int cordahip_commit_log_destroy(cordahip_ctx* ctx, uint32_t log_id);
/* grow + rehash on the device; a capacity_log2 at or below the current one changes nothing */
int cordahip_commit_log_reserve(cordahip_ctx* ctx, uint32_t log_id, uint32_t capacity_log2);
/* entries: live entries (exact); capacity: slots; next_seq: the sequence number of the next call's first transaction */
int cordahip_commit_log_stats(cordahip_ctx* ctx, uint32_t log_id, uint64_t* entries, uint64_t* capacity,
                              uint64_t* next_seq);
int cordahip_commit_log_load(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_row* rows, uint64_t n,
                             uint64_t* n_already_present);
/* present[n] (0 / 1), by[n] (zero rows where absent): the log as it stands after every call enqueued before */
int cordahip_commit_log_lookup(cordahip_ctx* ctx, uint32_t log_id, const cordahip_state_ref* refs, uint64_t n,
                               uint8_t* present, cordahip_consuming_tx* by);
/* Revoke: take back rows the caller could not persist (the database write failed while
 * the process lives -- what a rollback of the reference's JDBC-backed map does,
 * PersistentUniquenessProvider.kt:62-82). rows[i] = (ref, by) is a row as the caller was
 * about to persist it (cordahip_commit_log_load's shape; a ref listed twice carries its
 * LAST position). Row i removes the entry of `ref` iff the log holds `ref` and the stored
 * ConsumingTx equals `by` in all 40 bytes (id, input_index, caller): revoked[i] = 1.
 * Otherwise (absent ref, another id, position or caller) revoked[i] = 0 and the entry,
 * if any, is untouched. Equal rows repeated in one call all get 1 and remove the entry
 * once: *n_removed (may be NULL) counts entries, not rows. Loaded rows (sequence number
 * 0) are revocable on the same terms. Afterwards the log is, through every entry point,
 * the log into which the removed entries were never put: lookups say absent, the same
 * transaction commits again with committed = 1, another transaction spending the ref
 * commits, cordahip_commit_log_stats reports `entries` lower by *n_removed. next_seq does
 * not move, and the host's upper bound stays where it is until the next _stats call.
 * A host form (host pointers) that returns when done; it runs behind every call already
 * enqueued on the log, on any stream, and behind every ticket of
 * cordahip_commit_inputs_submit submitted before it. n == 0 is a successful no-op.
 * CORDAHIP_ERR_INVALID_ARG before any enqueue: NULL ctx, unknown or destroyed log id,
 * NULL rows / revoked with n > 0. */
int cordahip_commit_log_revoke(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_row* rows, uint64_t n,
                               uint8_t* revoked /* [n] out */, uint64_t* n_removed /* may be NULL */);
/* Export: the `snapshot` half of the replicated notaries' snapshot / install
 * (DistributedImmutableMap.kt:80-98, BFTSMaRt.kt:240-249; cordahip_commit_log_load is
 * install). Every live entry whose sequence number is >= since_seq (0: everything):
 * a loaded row carries 0, and transaction t of a commit call carries N + t, N being the
 * next_seq cordahip_commit_log_stats reported before that call -- so since_seq = a
 * next_seq read earlier exports exactly what the calls since then inserted (and nobody
 * revoked). *n_total is the number of matching entries; the first min(*n_total, cap)
 * slots of rows (and of seq, which may be NULL) are written and nothing beyond them.
 * *n_total > cap is not an error: size cap from _stats and call again; cap == 0 with
 * NULL rows only counts. THE ORDER OF THE ROWS IS UNSPECIFIED (it is neither insertion
 * nor sequence order, and differs between calls). Ordered on the log like revoke.
 * CORDAHIP_ERR_INVALID_ARG: NULL ctx or n_total, unknown log id, NULL rows with cap > 0. */
int cordahip_commit_log_export(cordahip_ctx* ctx, uint32_t log_id, uint64_t since_seq,
                               cordahip_commit_row* rows /* [cap] out */, uint64_t* seq /* [cap] out, may be NULL */,
                               uint64_t cap, uint64_t* n_total /* out */);

typedef struct {
  uint64_t ntx;
  const uint8_t* txid;            /* [ntx*32] */
  const uint32_t* caller;         /* [ntx] the JVM's id for the requesting Party; equal ids stand for equal Parties */
  const cordahip_state_ref* refs; /* [n_refs] */
  const uint64_t* tx_ref_off;     /* [ntx+1] into refs */
  uint64_t n_refs;
  const int64_t* tw_from;         /* [ntx] ns since the epoch, INT64_MIN = side absent; NULL with tw_until NULL: no windows */
  const int64_t* tw_until;
  int64_t now_ns, tolerance_ns;
  const uint8_t* gate;            /* [ntx] nonzero: skip; may be NULL */
  uint8_t* tx_status;             /* [ntx] out: OK / COMMIT_CONFLICT / COMMIT_TIME_WINDOW_INVALID / COMMIT_SKIPPED */
  uint8_t* committed;             /* [ntx] out: 1 = this call inserted the transaction's refs (the rows to persist) */
  uint8_t* ref_state;             /* [n_refs] out */
  cordahip_consuming_tx* ref_by;  /* [n_refs] out */
} cordahip_commit_batch;
int cordahip_commit_inputs(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_batch* batch);
int cordahip_commit_inputs_submit(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_batch* batch,
                                  uint64_t* ticket);
/* The device-resident form: `d_batch` is a HOST struct whose pointers are DEVICE
 * memory on the log's device (as cordahip_tx_cover_device takes its cover).
 * Stream-ordered on hip_stream; returns once enqueued. */
int cordahip_commit_inputs_device(cordahip_ctx* ctx, uint32_t log_id, const cordahip_commit_batch* d_batch,
                                  void* hip_stream);

/* ---- notary tear-offs from typed inputs and time windows (K21) ---------------------- *
 * What NonValidatingNotaryFlow.receiveAndVerifyTx does with a request
 * (NonValidatingNotaryFlow.kt:21-27): ftx.verify(), then commitInputStates over
 * ftx.filteredLeaves.inputs and .timeWindow -- the SAME objects whose serializedHash
 * verify() checked (MerkleTransaction.kt:69,135-140). NotaryFlow.Client reveals exactly
 * StateRefs and the TimeWindow (NotaryFlow.kt:62), so a tear-off arrives here as typed
 * rows: the cordahip_state_ref rows cordahip_commit_inputs takes, the window's two
 * Instants, the partial tree and the root. K21 hashes the rows' Kryo leaves on the GPU
 * (kinds STATE_REF / TIME_WINDOW above; bit-identical to SHA-256 of cordahip_kryo_encode's
 * leaf; no leaf bytes cross PCIe or touch HBM), K6 checks them against the partial tree,
 * and the commit form hands K16 the same device copies of the rows: the refs that are
 * committed are the refs that were proven. Leaf order is availableComponents order
 * (MerkleTransaction.kt:51-62): a transaction's refs in list order, then its window.
 * tx_status[t] is what cordahip_filtered_tx_verify answers for the same tear-off with
 * its leaves serialised by cordahip_kryo_encode -- OK, BAD_SIG, CORDAHIP_TX_NO_LEAVES
 * (no ref and no window), CORDAHIP_TX_BAD_TREE -- and CORDAHIP_TX_BAD_COMPONENT for a
 * window row that is no valid TIME_WINDOW item (its leaf hash is zero). The multiset
 * rule of PartialMerkleTree.verify (PartialMerkleTree.kt:132-139) is K6's: refs in
 * another order still verify; a tear-off that reveals any other component (a command)
 * cannot, as the typed form cannot name it. Both kinds are PARITY UNPINNED (see above).
 * tw_flags[t]: bit 7 the transaction has a TimeWindow; bits 0..6 the TIME_WINDOW item's
 * flags (bit 0 fromTime, bit 1 untilTime present); without bit 7 the row is ignored.
 * leaf_hash (may be NULL): the leaf hashes, packed, transaction by transaction -- leaf j
 * of transaction t at (tx_ref_off[t] - tx_ref_off[0]) + (windows before t) + j.
 * CSR: tx_ref_off[0..ntx] non-decreasing and within n_refs, tx_tok_off[0..ntx]
 * non-decreasing and within ntok, the five window arrays all given or all NULL: checked
 * whole before any enqueue, else CORDAHIP_ERR_INVALID_ARG (host forms). The verify
 * forms shard over the devices by transaction like cordahip_filtered_tx_verify. */
typedef struct {
  uint64_t ntx;
  const cordahip_state_ref* refs;  /* [n_refs] FilteredLeaves.inputs, list order */
  const uint64_t* tx_ref_off;      /* [ntx+1] */
  uint64_t n_refs;
  const uint8_t* tw_flags;         /* [ntx] bit 7: timeWindow present; bits 0/1 as the TIME_WINDOW item; NULL: no windows */
  const int64_t* tw_from_s;  const int32_t* tw_from_nano;    /* [ntx] */
  const int64_t* tw_until_s; const int32_t* tw_until_nano;   /* [ntx] */
  const uint8_t* tok; const uint8_t* tok_hash; const uint64_t* tx_tok_off; uint64_t ntok;  /* as cordahip_filtered_tx_batch */
  const uint8_t* root;             /* [ntx*32] FilteredTransaction.rootHash = the id */
  uint8_t* tx_status;              /* [ntx] out */
  uint8_t* leaf_hash;              /* [(n_refs + windows)*32] out, may be NULL */
} cordahip_notary_tearoff_batch;
int cordahip_notary_tearoff_verify(cordahip_ctx* ctx, const cordahip_notary_tearoff_batch* batch);
int cordahip_notary_tearoff_submit(cordahip_ctx* ctx, const cordahip_notary_tearoff_batch* batch, uint64_t* ticket);
/* The device-resident form: `d_batch` is a HOST struct whose pointers are DEVICE memory
 * on `device` (4-byte aligned; the int64 / uint64 arrays 8-byte aligned), stream-ordered
 * on hip_stream; returns once enqueued. d_tw_from / d_tw_until [ntx] int64 receive each
 * transaction's window as cordahip_commit_batch takes it: ns since the epoch as
 * seconds * 10^9 + nano, saturated at +-2^62, INT64_MIN for an absent side, an absent
 * window or an invalid window row. Offsets beyond n_refs are cut to n_refs on the
 * device, and a token range is read as given: tx_tok_off must lie within ntok. */
int cordahip_notary_tearoff_device(cordahip_ctx* ctx, int device, const cordahip_notary_tearoff_batch* d_batch,
                                   void* d_tw_from, void* d_tw_until, void* hip_stream);
/* Verify and commit in one call, wholly on the log's device and on one stream, no host
 * round trip between the stages: K21, K6, then K16 over the same device copies of refs /
 * tx_ref_off with txid = root, the windows K21 derived, and the gate (caller's gate[t]
 * != 0) OR (verify status != OK). batch->tx_status[t] is the verify status where that is
 * not OK, else K16's (OK / COMMIT_CONFLICT / COMMIT_TIME_WINDOW_INVALID / COMMIT_SKIPPED:
 * the two code sets do not overlap); it goes in as the signer's gate. caller, now_ns,
 * tolerance_ns, gate (may be NULL), committed, ref_state, ref_by (indexed like refs) and
 * the ordering on the log, CORDAHIP_ERR_LOG_FULL and the bound bookkeeping are
 * cordahip_commit_inputs's. */
int cordahip_notary_tearoff_commit(cordahip_ctx* ctx, uint32_t log_id, const cordahip_notary_tearoff_batch* batch,
                                   const uint32_t* caller, int64_t now_ns, int64_t tolerance_ns, const uint8_t* gate,
                                   uint8_t* committed, uint8_t* ref_state, cordahip_consuming_tx* ref_by);
int cordahip_notary_tearoff_commit_submit(cordahip_ctx* ctx, uint32_t log_id,
                                          const cordahip_notary_tearoff_batch* batch, const uint32_t* caller,
                                          int64_t now_ns, int64_t tolerance_ns, const uint8_t* gate, uint8_t* committed,
                                          uint8_t* ref_state, cordahip_consuming_tx* ref_by, uint64_t* ticket);

/* ---- a full transaction's inputs and time window as commit rows (K22) ---------------- *
 * A validating notary (ValidatingNotaryFlow) and any node that commits what it
 * resolved see the whole transaction: its inputs are the STATE_REF items, and its window
 * the TIME_WINDOW item, of the very component batch whose id and signatures
 * cordahip_signed_txcomp_verify_ed25519_device has just computed and checked. This call
 * takes them out of those items in HBM as the rows cordahip_commit_inputs_device takes,
 * so the refs that are committed are the refs that were hashed into the id, and nothing
 * is read back to the host in between:
 *   components -> ids -> signatures -> (coverage) -> inputs and window -> commit -> sign
 * d_items, d_payload and d_tx_item_off are exactly what
 * cordahip_signed_txcomp_verify_ed25519_device takes (items[i].data OFFSETS into
 * d_payload). Per transaction t, its item range cut to n_items (the offsets are
 * untrusted; a reversed range is empty):
 *   inputs  its STATE_REF items in item order, copied as 36-byte cordahip_state_ref
 *           rows to d_refs at d_tx_ref_off[t]. d_tx_ref_off[t] is the running count of
 *           refs clamped to ref_cap, d_tx_ref_off[ntx] the clamped total. A STATE_REF
 *           item whose len != 36 or whose payload runs past payload_len flags the
 *           transaction.
 *   window  no TIME_WINDOW item: both sides INT64_MIN. Exactly one valid item (as
 *           CORDAHIP_KRYO_TIME_WINDOW defines valid): each present side as
 *           cordahip_commit_batch takes it, seconds * 10^9 + nano saturated at +-2^62,
 *           INT64_MIN for an absent side. Two or more TIME_WINDOW items, an invalid
 *           row or a payload out of range flag the transaction.
 *   A transaction flagged by its items has an empty ref range and both window sides
 *   INT64_MIN. A transaction whose unclamped ref range ends beyond ref_cap is flagged
 *   too and its range is cut at ref_cap; nothing is written at or past d_refs[ref_cap].
 *   gate    d_gate[t] = d_tx_status[t] if that is given and nonzero, else
 *           CORDAHIP_TX_BAD_COMPONENT if the transaction is flagged, else 0. It goes in
 *           as cordahip_commit_batch.gate. cordahip_tx_cover_device rewrites
 *           d_tx_status in place: run before this call it brings required-signer
 *           coverage into the gate.
 * Items of every other kind are skipped; a transaction with no STATE_REF item (an
 * issue) has an empty range, which cordahip_commit_inputs commits as a transaction
 * with no inputs. d_refs is 4-byte aligned, the 64-bit arrays 8-byte aligned; d_gate is
 * an array of its own (not d_tx_status).
 * CORDAHIP_ERR_INVALID_ARG before any enqueue: NULL ctx, unknown device, a NULL or
 * misaligned output or NULL d_tx_item_off with ntx > 0, NULL d_items with n_items > 0,
 * NULL d_refs with ref_cap > 0, n_items >= 2^31 - 1. Stream-ordered on hip_stream;
 * returns once enqueued; ntx == 0 is a successful no-op. No device scratch. */
int cordahip_txcomp_inputs_device(cordahip_ctx* ctx, int device, const void* d_items, uint64_t n_items,
                                  const void* d_payload, uint64_t payload_len, const void* d_tx_item_off, uint64_t ntx,
                                  const void* d_tx_status /* uint8[ntx] or NULL */,
                                  void* d_refs, uint64_t ref_cap /* cordahip_state_ref[ref_cap] out */,
                                  void* d_tx_ref_off /* uint64[ntx+1] out */,
                                  void* d_tw_from, void* d_tw_until /* int64[ntx] out */,
                                  void* d_gate /* uint8[ntx] out */, void* hip_stream);

/* Device time (ms) of the calling thread's most recent *_device call on
 * `device`, from HIP events recorded around its launches on the stream it ran
 * on (waits for them); -1 if the thread made no such call. Each call gets its
 * own event pair from a per-device ring of 64, so concurrent callers on other
 * threads or streams do not disturb it -- up to 64 calls on the device in
 * between: after more, the slot has been reused and the result is -1. */
double cordahip_last_kernel_ms(cordahip_ctx* ctx, int device);

/* The in-process partition rule: shard `shard` of `nshards` over n lanes is
 * [*lo, *hi), contiguous, 64-aligned starts (whole verdict words), the last
 * shard possibly short or empty. Every multi-device host path uses it (per
 * scheme for generic batches; per transaction for tx batches, align 1). */
void cordahip_shard_range(uint64_t n, uint32_t nshards, uint32_t shard, uint64_t align, uint64_t* lo, uint64_t* hi);

#ifdef __cplusplus
}
#endif
#endif /* CORDAHIP_H */
