"""Batched transaction resolution: the signature and transaction-id half of
ResolveTransactionsFlow / FinalityFlow / SignedTransaction.verifySignatures
 over ONE submission to the engine.

Reference call chain today (serial on the Node thread, one JCA call per
signature, every signature checked twice):

  ResolveTransactionsFlow.call                core/.../flows/ResolveTransactionsFlow.kt:97-131
    topologicalSort(downloaded)               :40-66
    for stx in newTxns:                       :106-114
      stx.toLedgerTransaction(serviceHub)     core/.../transactions/SignedTransaction.kt:155-159
        checkSignaturesAreValid()             :95-100   first invalid signature throws
        verifySignatures()                    :70-85    checkSignaturesAreValid() AGAIN, then
                                                        getMissingSignatures() :102-108 ->
                                                        SignaturesMissingException :54-55, :81
      transactionVerifierService.verify(ltx)  contract logic: out of scope (a hook here)
      recordTransactions(stx)

Here every transaction's id (K3/K4) and every signature (K1/K2) go to the GPU
in one cordahip_signed_tx_verify call (Engine.signed_tx_verify), each
signature is verified once, and the host then walks the topological order
raising exactly the exception the Kotlin loop would raise first. The JVM side
of this (the Kotlin a maintainer adds) is sketched in INTEGRATION.md §3.
"""
from __future__ import annotations

import os

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple, Union

# per-lane statuses of include/cordahip.h
OK, BAD_SIG, MALFORMED_SIG, BAD_KEY, UNSUPPORTED, EMPTY = 0, 1, 2, 3, 4, 5
TX_NO_LEAVES, TX_NO_SIGNATURES = 6, 7
TX_SIGNATURES_MISSING, TX_BAD_COVER = 10, 11  # required-signer coverage (cordahip_cover)
REQ_MISSING = 1
TX_HASHES_NOT_IN_TREE = 12  # FilteredTransaction build: the count rule (PartialMerkleTree.kt:75-76)
_SIGN_UNKNOWN_KEY = 14  # cordahip_sign: the lane's key id names no live key
_VERIFY_UNKNOWN_KEY = 16  # cordahip_verify_keyed: the lane's key id names no live verification key


class SignatureException(Exception):
    """java.security.SignatureException"""


class SignaturesMissingException(SignatureException):
    """SignedTransaction.SignaturesMissingException (SignedTransaction.kt:54-55)."""

    def __init__(self, missing, descriptions, tx_id: bytes):
        super().__init__("Missing signatures for %s on transaction %s" % (descriptions, tx_id.hex()[:6].upper()))
        self.missing, self.descriptions, self.id = missing, descriptions, tx_id


class IllegalArgumentException(Exception):
    """java.lang.IllegalArgumentException (require failures, unsupported schemes, bad keys)."""


class NoSuchElementException(Exception):
    """java.util.NoSuchElementException (the KMS holds no key pair for the key asked for:
    `publicKey.keys.first { keys.containsKey(it) }`, PersistentKeyManagementService.kt:80-85)."""


class MerkleTreeException(Exception):
    """MerkleTreeException: a transaction with no components (MerkleTree.kt:49-50)."""


class TransactionGraphException(IllegalArgumentException):
    """topologicalSort's require(result.size == transactions.size) (ResolveTransactionsFlow.kt:64)."""


@dataclass(frozen=True)
class CompositeKey:
    """CompositeKey (core/.../crypto/composite/CompositeKey.kt:35): a threshold tree whose
    leaves are encoded public keys (bytes) and whose inner nodes are CompositeKeys."""
    threshold: int
    children: Tuple[Tuple[Union[bytes, "CompositeKey"], int], ...]  # (node, weight)

    def is_fulfilled_by(self, keys) -> bool:
        # checkFulfilledBy, CompositeKey.kt:186-196
        total = sum(w for node, w in self.children if is_fulfilled_by(node, keys))
        return total >= self.threshold


def is_fulfilled_by(key, keys) -> bool:
    """PublicKey.isFulfilledBy(otherKeys), CryptoUtils.kt:79-82."""
    return key.is_fulfilled_by(keys) if isinstance(key, CompositeKey) else key in keys


@dataclass
class SignedTx:
    """What SignedTransaction holds for the path: the serialised available components
    (the Merkle leaves, MerkleTransaction.kt:51-62), the signatures in list order as
    DigitalSignature.WithKey (scheme, encoded key, signature bytes), tx.mustSign, and
    tx.inputs' transaction hashes (for topologicalSort)."""
    components: List[bytes]
    sigs: List[Tuple[int, bytes, bytes]]
    must_sign: List[Union[bytes, CompositeKey]] = field(default_factory=list)
    inputs: List[bytes] = field(default_factory=list)
    # for getMissingKeyDescriptions (SignedTransaction.kt:114-124): tx.commands as
    # (command.toString(), signers) and tx.notary?.owningKey
    commands: List[Tuple[str, List[Union[bytes, CompositeKey]]]] = field(default_factory=list)
    notary: Optional[Union[bytes, CompositeKey]] = None


def _lane_exception(status: int) -> Exception:
    """Per-lane status -> the exception Crypto.doVerify / the key decoder throws
    (INTEGRATION.md §1 table)."""
    if status == BAD_SIG:
        return SignatureException("Signature Verification failed!")  # Crypto.kt:481
    if status == MALFORMED_SIG:
        return SignatureException("error decoding signature bytes.")  # engine-level (JCA)
    if status == BAD_KEY:
        return IllegalArgumentException("invalid public key")  # key decode (Kryo.kt:389-392, Crypto.kt:353)
    if status == UNSUPPORTED:
        return IllegalArgumentException("Unsupported key/algorithm")  # Crypto.kt:474
    if status == EMPTY:
        return IllegalArgumentException("Signature data is empty!")  # Crypto.kt:475-476
    raise ValueError("status %d is not an exception" % status)


@dataclass
class Outcome:
    id: Optional[bytes]                 # WireTransaction.id (None when it cannot be computed)
    error: Optional[Exception]          # what verifySignatures() throws first, or None
    first_bad_sig: int = -1             # index in stx.sigs of the signature that threw


def missing_key_descriptions(stx: SignedTx, missing) -> List[str]:
    """getMissingKeyDescriptions (SignedTransaction.kt:114-124): every command with a
    missing signer (command.toString(), in command order), then "notary" if the
    notary's key is missing."""
    miss = set(missing)
    out = [desc for desc, signers in stx.commands if any(k in miss for k in signers)]
    if stx.notary is not None and stx.notary in miss:
        out.append("notary")
    return out


def verify_signatures_batch(engine, stxs: Sequence[SignedTx], allowed_to_be_missing=()) -> List[Outcome]:
    """SignedTransaction.verifySignatures(*allowed_to_be_missing) for every stx, one engine call.

    Exception precedence per transaction follows the Kotlin code: the
    constructor's require(sigs.isNotEmpty()) (:37-39), then tx.id (MerkleTree),
    then the signatures in list order (:95-100), then the missing signers
    (:76-82, minus allowed_to_be_missing)."""
    if not stxs:
        return []
    ids, tx_st, first_bad, _ = engine.signed_tx_verify([s.components for s in stxs], [s.sigs for s in stxs])
    allowed = set(allowed_to_be_missing)
    out = []
    for t, stx in enumerate(stxs):
        st = int(tx_st[t])
        if st == TX_NO_SIGNATURES:
            out.append(Outcome(None, IllegalArgumentException("Failed requirement.")))
            continue
        if st == TX_NO_LEAVES:
            out.append(Outcome(None, MerkleTreeException("Cannot calculate Merkle root on empty hash list.")))
            continue
        tid = bytes(ids[t])
        if st != OK:
            out.append(Outcome(tid, _lane_exception(st), int(first_bad[t])))
            continue
        sig_keys = {k for _, k, _ in stx.sigs}
        # getMissingSignatures (:102-108): mustSign.filter { !isFulfilledBy }.toSet() -- a
        # LinkedHashSet, so duplicates collapse and list order is kept; `missing - allowed`
        # (:79) keeps that order too
        missing = dict.fromkeys(k for k in stx.must_sign if not is_fulfilled_by(k, sig_keys))
        needed = [k for k in missing if k not in allowed]
        if needed:
            out.append(Outcome(tid, SignaturesMissingException(needed, missing_key_descriptions(stx, needed), tid)))
            continue
        out.append(Outcome(tid, None))
    return out


def verify_signatures_batch_covered(engine, stxs: Sequence[SignedTx], allowed_to_be_missing=()) -> List[Outcome]:
    """verify_signatures_batch with getMissingSignatures (:102-108) done by the library too
    (engine.signed_tx_verify_covered: one call is the whole of verifySignatures). Only the set
    semantics (.toSet(), list order kept) and the descriptions are rebuilt here, from
    req_status. A required key that CompositeKey.checkValidity (CompositeKey.kt:110-122)
    rejects is an IllegalArgumentException, thrown before any missing set exists."""
    if not stxs:
        return []
    from . import cover as C
    cov = C.flatten([s.must_sign for s in stxs], [s.sigs for s in stxs], allowed_to_be_missing)
    ids, tx_st, first_bad, _, req_st, _ = engine.signed_tx_verify_covered([s.components for s in stxs],
                                                                         [s.sigs for s in stxs], cov)
    out = []
    for t, stx in enumerate(stxs):
        st = int(tx_st[t])
        if st == TX_NO_SIGNATURES:
            out.append(Outcome(None, IllegalArgumentException("Failed requirement.")))
            continue
        if st == TX_NO_LEAVES:
            out.append(Outcome(None, MerkleTreeException("Cannot calculate Merkle root on empty hash list.")))
            continue
        tid = bytes(ids[t])
        if st == TX_BAD_COVER:
            out.append(Outcome(tid, IllegalArgumentException("invalid CompositeKey")))
        elif st == TX_SIGNATURES_MISSING:
            r0 = int(cov.tx_req_off[t])
            needed = list(dict.fromkeys(k for i, k in enumerate(stx.must_sign) if req_st[r0 + i] == REQ_MISSING))
            out.append(Outcome(tid, SignaturesMissingException(needed, missing_key_descriptions(stx, needed), tid)))
        elif st != OK:
            out.append(Outcome(tid, _lane_exception(st), int(first_bad[t])))
        else:
            out.append(Outcome(tid, None))
    return out


def build_filtered_transactions(engine, wtxs, filtering: Callable[[bytes], bool]):
    """WireTransaction.buildFilteredTransaction(filtering) (WireTransaction.kt, via
    FilteredTransaction.buildMerkleTransaction, MerkleTransaction.kt:121-128) for every
    transaction, one engine call (Engine.filtered_tx_build: K3 leaf hashes, K10 trees).

    wtxs[t]: a SignedTx or the transaction's serialised components (the Merkle leaves) in
    availableComponents order; filtering(component) is the predicate filterWithFun applies to
    each of them. Returns per transaction (filtered leaves, tokens, root): the FilteredLeaves'
    components in order, the PartialMerkleTree's post-order tokens and rootHash -- the tuple
    Engine.filtered_tx_verify takes. Like a loop over the Kotlin call, the first transaction
    (input order) whose build throws raises: MerkleTreeException for a transaction with no
    components (MerkleTree.kt:49-50) and for included hashes the tree does not hold one to one
    (PartialMerkleTree.kt:75-76: an unselected component equal to a selected one)."""
    comps = [list(w.components) if isinstance(w, SignedTx) else list(w) for w in wtxs]
    if not comps:
        return []
    masks = [[bool(filtering(c)) for c in cs] for cs in comps]
    ids, status, toks = engine.filtered_tx_build(list(zip(comps, masks)))
    out = []
    for t, cs in enumerate(comps):
        st = int(status[t])
        if st == TX_NO_LEAVES:
            raise MerkleTreeException("Cannot calculate Merkle root on empty hash list.")
        if st == TX_HASHES_NOT_IN_TREE:
            raise MerkleTreeException("Some of the provided hashes are not in the tree.")
        if st != OK:
            raise RuntimeError("filtered_tx_build: transaction %d has status %d" % (t, st))
        out.append(([c for c, f in zip(cs, masks[t]) if f], toks[t], bytes(ids[t])))
    return out


def _sign_with(engine, key_id: int, msgs, gate, salts=None):
    """One signing call over msgs with the registered key `key_id`, gated: Engine.sign_batch for an
    Ed25519 signer id, Engine.ecdsa_sign_batch for an ECDSA one, Engine.rsa_sign_batch for an RSA
    one (Engine.signer_family). An RSA signature needs a 32-byte salt per lane: `salts`, else
    os.urandom -- the JVM's SecureRandom in this mirror. Returns (sigs, status): sigs[t] the
    signature bytes -- 64 bytes R || S, the DER bytes of an ECDSA signature, or the k bytes of an
    RSA one -- for a lane whose status is OK."""
    family = getattr(engine, "signer_family", lambda k: None)(key_id)
    if family == "rsa":
        if salts is None:
            salts = [os.urandom(32) for _ in msgs]
        rows, lens, sst = engine.rsa_sign_batch([key_id] * len(msgs), msgs, salts, gate=gate)
        return [bytes(rows[t][:int(lens[t])]) for t in range(len(msgs))], sst
    if family in (2, 3):
        rows, lens, sst = engine.ecdsa_sign_batch([key_id] * len(msgs), msgs, gate=gate)
        return [bytes(rows[t][:int(lens[t])]) for t in range(len(msgs))], sst
    rows, sst = engine.sign_batch([key_id] * len(msgs), msgs, gate=gate)
    return [bytes(r) for r in rows], sst


def verify_and_sign_filtered_transactions(engine, ftxs, key_id: int):
    """What an oracle or a non-validating notary does with a batch of tear-offs
    (NodeInterestRates.sign, NodeInterestRates.kt:149-180: ftx.verify(), then
    keyManagementService.sign(ftx.rootHash.bytes, signingKey); NotaryFlow.Service,
    NotaryFlow.kt:114-116): Engine.filtered_tx_verify over ftxs (the tuples it takes),
    then one signing call over the root hashes with the registered key `key_id` (Ed25519:
    Engine.sign_batch; an ECDSA signer id: Engine.ecdsa_sign_batch), gated on the
    verification statuses -- a tear-off that did not verify is not signed.

    Returns (tx_status, sigs): tx_status[t] as filtered_tx_verify gives it, sigs[t] the
    signature over ftxs[t]'s root (64 bytes for an Ed25519 key, DER for an ECDSA key), or
    None where tx_status[t] != OK. An id that
    names no live key raises NoSuchElementException, as the KMS's key lookup does
    (PersistentKeyManagementService.kt:80-89)."""
    if not ftxs:
        return [], []
    status = engine.filtered_tx_verify(ftxs)
    sigs, sst = _sign_with(engine, key_id, [bytes(f[2]) for f in ftxs], status)
    out = []
    for t in range(len(ftxs)):
        if int(sst[t]) == _SIGN_UNKNOWN_KEY:
            raise NoSuchElementException("no registered key %d" % key_id)
        out.append(bytes(sigs[t]) if int(sst[t]) == OK else None)
    return [int(x) for x in status], out


_COMMIT_CONFLICT, _COMMIT_TIME_WINDOW_INVALID = 16, 17  # cordahip_commit_inputs tx statuses


@dataclass
class NotaryError:
    """NotaryError (NotaryFlow.kt): kind is "TransactionInvalid", "TimeWindowInvalid" or "Conflict";
    a Conflict carries tx_id and state_history = {(txhash, index): (txid, input_index, caller)},
    the consumed inputs in input order (first occurrence of a ref), as the reference's signed
    UniquenessProvider.Conflict lists them."""
    kind: str
    tx_id: Optional[bytes] = None
    state_history: dict = field(default_factory=dict)


def time_window_valid(window, now_ns: int, tolerance_ns: int) -> bool:
    """TimeWindowChecker.isValid (TimeWindowChecker.kt:14-25) in exact nanoseconds: window None or
    (from_ns or None, until_ns or None); invalid iff now - until > tolerance or from - now > tolerance."""
    if window is None:
        return True
    lo, hi = window
    return not ((hi is not None and now_ns - hi > tolerance_ns) or (lo is not None and lo - now_ns > tolerance_ns))


def commit_input_states(log: dict, txs, now_ns: int = 0, tolerance_ns: int = 0, gate=None):
    """The pure-Python mirror of Engine.commit_inputs: TrustedAuthorityNotaryService.validateTimeWindow
    and commitInputStates (NotaryService.kt:44-47, :53-67) over PersistentUniquenessProvider.commit
    (PersistentUniquenessProvider.kt:62-82), one transaction at a time in batch order against `log`
    = {(txhash, index): (txid, input_index, caller)}, which it updates. txs and the result are
    Engine.commit_inputs's: (tx_status, committed, ref_state, ref_by)."""
    status, committed, states, bys = [], [], [], []
    for t, (txid, caller, refs, window) in enumerate(txs):
        txid, caller = bytes(txid), int(caller)
        keys = [(bytes(h), int(i)) for h, i in refs]
        st, cm = OK, 0
        rs, rb = [0] * len(keys), [None] * len(keys)
        if gate is not None and gate[t]:
            st = 18
        elif not time_window_valid(window, now_ns, tolerance_ns):
            st = _COMMIT_TIME_WINDOW_INVALID
        else:
            history = {k: log[k] for k in keys if k in log}  # UniquenessProvider.Conflict.stateHistory
            if not history:
                for i, k in enumerate(keys):
                    log[k] = (txid, i, caller)
                cm = 1
            else:
                for i, k in enumerate(keys):
                    if k in history:
                        rb[i] = history[k]
                        rs[i] = 1 if history[k] == (txid, i, caller) else 2
                if 2 in rs:
                    st = _COMMIT_CONFLICT
        status.append(st)
        committed.append(cm)
        states.append(rs)
        bys.append(rb)
    return status, committed, states, bys


def notarise_filtered_transactions(engine, log_id: int, ftxs, inputs, time_windows, callers, key_id: int,
                                   now: int, tolerance: int):
    """The batch form of NotaryFlow.Service.call (NotaryFlow.kt:98-104) for a non-validating notary:
    Engine.filtered_tx_verify over the tear-offs (ftx.verify()), Engine.commit_inputs gated on its
    statuses (validateTimeWindow, commitInputStates, in batch order against the commit log `log_id`),
    Engine.sign_batch (Engine.ecdsa_sign_batch for an ECDSA signer id) over the root hashes gated on
    the commit statuses (service.sign(txId.bytes)).

    ftxs[t]: the tuple filtered_tx_verify takes, its root the transaction id; inputs[t]: the
    tear-off's input StateRefs [(txhash, index)]; time_windows[t]: None or (from_ns or None, until_ns
    or None); callers[t]: the requesting party's id; now / tolerance in ns.

    Returns (answers, committed_rows). answers[t] is the signature (64 bytes; DER for an ECDSA key), or the NotaryError the
    reference sends: TransactionInvalid for a tear-off that does not verify, TimeWindowInvalid,
    Conflict with its state history. committed_rows lists ((txhash, index), (txid, input_index,
    caller)) for every input state this call consumed -- what the caller persists BEFORE it releases
    the signatures (a ref listed twice once, with the position the log stores: its last)."""
    n = len(ftxs)
    assert len(inputs) == len(time_windows) == len(callers) == n
    if n == 0:
        return [], []
    ids = [bytes(f[2]) for f in ftxs]
    verified = engine.filtered_tx_verify(ftxs)
    txs = [(ids[t], callers[t], list(inputs[t]), time_windows[t]) for t in range(n)]
    status, committed, ref_state, ref_by = engine.commit_inputs(log_id, txs, now, tolerance, gate=verified)
    sigs, sst = _sign_with(engine, key_id, ids, status)
    answers, rows = [], []
    for t in range(n):
        st = int(status[t])
        if int(verified[t]) != OK:
            answers.append(NotaryError("TransactionInvalid", ids[t]))
        elif st == _COMMIT_TIME_WINDOW_INVALID:
            answers.append(NotaryError("TimeWindowInvalid", ids[t]))
        elif st == _COMMIT_CONFLICT:
            hist = {}
            for r, by in zip(inputs[t], ref_by[t]):
                if by is not None:
                    hist.setdefault((bytes(r[0]), int(r[1])), by)
            answers.append(NotaryError("Conflict", ids[t], hist))
        elif int(sst[t]) == _SIGN_UNKNOWN_KEY:
            raise NoSuchElementException("no registered key %d" % key_id)
        else:
            answers.append(bytes(sigs[t]))
        if committed[t]:
            last = {}
            for i, r in enumerate(inputs[t]):
                last[(bytes(r[0]), int(r[1]))] = (ids[t], i, int(callers[t]))
            rows.extend(last.items())
    return answers, rows


def notarise_filtered_transactions_persisted(engine, log_id: int, ftxs, inputs, time_windows, callers, key_id: int,
                                             now: int, tolerance: int, persist):
    """notarise_filtered_transactions with the database write inside the call, as the reference's
    commit runs inside the flow's database transaction (PersistentUniquenessProvider.kt:62-82 over
    AbstractJDBCHashMap): persist(committed_rows) is called before anything is returned. If it
    raises, exactly those rows are revoked (Engine.commit_log_revoke: the log is again the log the
    database describes, every row must have been revoked) and the exception is re-raised -- no
    answer, and so no signature, leaves the call. Answers of a later batch on the same log must not
    be released while this one's rows are neither persisted nor revoked.

    Returns (answers, committed_rows) as notarise_filtered_transactions does."""
    answers, rows = notarise_filtered_transactions(engine, log_id, ftxs, inputs, time_windows, callers, key_id,
                                                   now, tolerance)
    try:
        persist(rows)
    except BaseException:
        revoked, removed = engine.commit_log_revoke(log_id, rows)
        assert all(revoked) and removed == len(rows), "rows of a failed write that the log no longer holds"
        raise
    return answers, rows


_COMMIT_STATUSES = (OK, _COMMIT_CONFLICT, _COMMIT_TIME_WINDOW_INVALID, 18)  # what K16 answers; the rest are verify statuses


def notarise_tearoffs(engine, log_id: int, tearoffs, callers, key_id: int, now: int, tolerance: int):
    """notarise_filtered_transactions for tear-offs given as TYPED components, the way
    NonValidatingNotaryFlow.receiveAndVerifyTx uses them (NonValidatingNotaryFlow.kt:21-27): the
    refs and the window that are committed are the ones ftx.verify() hashed, not separate arguments.
    tearoffs[t] = (refs, window, tokens, root): refs = [(txhash, index)] (FilteredLeaves.inputs),
    window None or (from, until) with a side None or (epochSecond, nano) (FilteredLeaves.timeWindow),
    tokens the partial tree as filtered_tx_verify takes it, root the transaction id. One
    Engine.notary_tearoff_commit (K21 + K6 + K16 on the log's device, no leaf serialised anywhere),
    then the signing call gated on its statuses.

    Returns (answers, committed_rows) exactly as notarise_filtered_transactions does for the same
    tear-offs with their leaves serialised and the same refs and windows; a window row that is no
    Instant pair (CORDAHIP_TX_BAD_COMPONENT) is a TransactionInvalid."""
    n = len(tearoffs)
    assert len(callers) == n
    if n == 0:
        return [], []
    ids = [bytes(f[3]) for f in tearoffs]
    status, committed, ref_state, ref_by = engine.notary_tearoff_commit(log_id, tearoffs, callers, now, tolerance)
    sigs, sst = _sign_with(engine, key_id, ids, status)
    answers, rows = [], []
    for t in range(n):
        st = int(status[t])
        refs = tearoffs[t][0]
        if st not in _COMMIT_STATUSES:
            answers.append(NotaryError("TransactionInvalid", ids[t]))
        elif st == _COMMIT_TIME_WINDOW_INVALID:
            answers.append(NotaryError("TimeWindowInvalid", ids[t]))
        elif st == _COMMIT_CONFLICT:
            hist = {}
            for r, by in zip(refs, ref_by[t]):
                if by is not None:
                    hist.setdefault((bytes(r[0]), int(r[1])), by)
            answers.append(NotaryError("Conflict", ids[t], hist))
        elif int(sst[t]) == _SIGN_UNKNOWN_KEY:
            raise NoSuchElementException("no registered key %d" % key_id)
        else:
            answers.append(bytes(sigs[t]))
        if committed[t]:
            last = {}
            for i, r in enumerate(refs):
                last[(bytes(r[0]), int(r[1]))] = (ids[t], i, int(callers[t]))
            rows.extend(last.items())
    return answers, rows


def notarise_tearoffs_persisted(engine, log_id: int, tearoffs, callers, key_id: int, now: int, tolerance: int, persist):
    """notarise_tearoffs with the database write inside the call, on the terms of
    notarise_filtered_transactions_persisted: persist(committed_rows) before anything is returned;
    if it raises, exactly those rows are revoked and the exception is re-raised."""
    answers, rows = notarise_tearoffs(engine, log_id, tearoffs, callers, key_id, now, tolerance)
    try:
        persist(rows)
    except BaseException:
        revoked, removed = engine.commit_log_revoke(log_id, rows)
        assert all(revoked) and removed == len(rows), "rows of a failed write that the log no longer holds"
        raise
    return answers, rows


def notarise_transactions(engine, log_id: int, stxs_as_components, callers, key_id: int, now: int, tolerance: int,
                          device: int = 0, stream=None, detail: Optional[dict] = None, notary_family: str = "ed25519",
                          salts=None):
    """What a VALIDATING notary (ValidatingNotaryFlow) or any node that commits what it resolved does
    with full transactions, on torch device tensors and ONE stream, with no device-to-host copy
    before the final download (K22):
      1. Engine.signed_txcomp_verify_ed25519_device  components -> ids -> signature verdicts
      2. Engine.txcomp_inputs_device                 the STATE_REF / TIME_WINDOW items of the same
                                                     device batch -> refs, offsets, windows, gate
      3. Engine.commit_inputs_device                 txid = the ids of step 1, gated
      4. Engine.ed25519_sign_keyed_device            over the ids, gated by the commit status
    so the inputs that are committed are the components whose hashes made the id that was signed.
    Contract verification and required-signer coverage (Engine.tx_cover_device between steps 1
    and 2) are the caller's.

    stxs_as_components[t] = (components, sigs): components as (kind, value, class_id) tuples
    (_lib.kryo_pack's form, availableComponents order), sigs = [(key 32 bytes, signature 64 bytes)]
    -- Ed25519 pairs, the dense path above -- or (scheme, key, sig) triples of any scheme (K23). When
    any triple is present, step 1 is Engine.signed_txcomp_verify_device over all of the batch's
    signatures (a pair counts as an Ed25519 triple): classified and packed on the GPU, RSA_SHA256
    following Engine.set_rsa_on_device. notary_family: "ed25519" (step 4 as above, 64-byte answers)
    or "ecdsa" (key_id is an ECDSA signer's: Engine.ecdsa_sign_keyed_device, DER answers) or "rsa"
    (K24: key_id is an RSA signer's and salts[t] the caller-drawn 32-byte salt of transaction t, as
    Engine.rsa_sign_keyed_device takes them; the call is enqueued once per width class, a key answers
    in its own; the answers are the signature bytes at their sig_len). salts without "rsa", or "rsa"
    without salts, is an AssertionError.
    Registered verification keys: with the family switches and Engine.vkey_set_routing_device on,
    the mixed step 1 sends the signatures of registered keys to the keyed verifiers; the answers
    and the committed rows are those of the unrouted call.
    callers[t]: the requesting party's id; now / tolerance in ns; `device` is the log's.

    Returns (answers, committed_rows) in notarise_tearoffs's shape: answers[t] the notary's signature
    over the id, or NotaryError -- TransactionInvalid (tx_id None where the id could not be
    computed) for a transaction whose signatures or components do not verify, TimeWindowInvalid,
    Conflict with its state history. detail, if given, receives the raw arrays: ids, status (the
    verify status where that is not OK, else the commit's), committed, refs, tx_ref_off."""
    import numpy as np
    import torch

    from corda_amd import _lib
    n = len(stxs_as_components)
    assert len(callers) == n
    if n == 0:
        return [], []
    dev = torch.device("cuda", device)
    s = stream if stream is not None else torch.cuda.Stream(dev)
    blob, items, has = _lib.kryo_pack([c for comps, _ in stxs_as_components for c in comps])
    items = items.copy()
    items["data"] = np.where(has, items["data"], 0)  # offsets into the payload
    tio = np.zeros(n + 1, np.int64)
    tio[1:] = np.cumsum([len(comps) for comps, _ in stxs_as_components])
    tso = np.zeros(n + 1, np.int64)
    tso[1:] = np.cumsum([len(sg) for _, sg in stxs_as_components])
    assert notary_family in ("ed25519", "ecdsa", "rsa")
    assert (salts is not None) == (notary_family == "rsa"), "salts go with notary_family='rsa', and only with it"
    if salts is not None:
        assert len(salts) == n and all(len(x) == 32 for x in salts)
    flat = [x for _, sg in stxs_as_components for x in sg]
    mixed = any(len(x) == 3 for x in flat)
    if mixed:  # every signature as a (scheme, key, sig) triple, CSR
        flat = [x if len(x) == 3 else (4, x[0], x[1]) for x in flat]
        sch = np.asarray([x[0] for x in flat], np.uint8)
        key_off, sig_off = np.zeros(len(flat) + 1, np.int64), np.zeros(len(flat) + 1, np.int64)
        key_off[1:] = np.cumsum([len(x[1]) for x in flat])
        sig_off[1:] = np.cumsum([len(x[2]) for x in flat])
        keys = np.frombuffer(b"".join(bytes(x[1]) for x in flat), np.uint8)
        sigs = np.frombuffer(b"".join(bytes(x[2]) for x in flat), np.uint8)
    else:
        assert all(len(k) == 32 and len(g) == 64 for k, g in flat), "Ed25519 keys and signatures only"
        keys = np.frombuffer(b"".join(bytes(k) for k, _ in flat) or bytes(32), np.uint8).reshape(-1, 32)
        sigs = np.frombuffer(b"".join(bytes(g) for _, g in flat) or bytes(64), np.uint8).reshape(-1, 64)
    nsig, n_items = len(flat), len(items)
    ref_cap = int((items["kind"] == _lib.KRYO_KINDS["state_ref"]).sum())
    with torch.cuda.stream(s):
        up = lambda a: torch.from_numpy(np.array(a, copy=True)).to(dev)  # noqa: E731
        z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        d_items = up(items.view(np.uint8).reshape(-1, _lib.KRYO_ITEM_DTYPE.itemsize)) if n_items else z(1, 32)
        d_blob, d_tio, d_tso = up(blob), up(tio), up(tso)
        if mixed:
            d_sch, d_keys, d_sigs, d_key_off, d_sig_off = up(sch), up(keys), up(sigs), up(key_off), up(sig_off)
        else:
            d_keys, d_sigs = up(keys)[:max(nsig, 1)], up(sigs)[:max(nsig, 1)]
        d_caller = up(np.asarray(callers, np.int32))
        d_key_id = torch.full((n,), key_id, dtype=torch.int32, device=dev)
        txid, v_status, first_bad, sig_status = z(n, 32), z(n), z(n, dt=torch.int64), z(max(nsig, 1))
        refs, tx_ref_off = z(max(ref_cap, 1), 36), z(n + 1, dt=torch.int64)
        tw_from, tw_until, gate = z(n, dt=torch.int64), z(n, dt=torch.int64), z(n)
        c_status, committed = z(n), z(n)
        ref_state, ref_by = z(max(ref_cap, 1)), z(max(ref_cap, 1), 40)
        ecdsa_notary, rsa_notary = notary_family == "ecdsa", notary_family == "rsa"
        n_sigs, n_sig_len, s_status = z(n, 72 if ecdsa_notary else 64), z(n), z(n)
        if rsa_notary:  # a slot, a length and a status per width class
            d_salts = up(np.frombuffer(b"".join(bytes(x) for x in salts), np.uint8).reshape(n, 32))
            rsa_out = [(z(n, 4 * w), z(n, dt=torch.int16), z(n)) for w in (64, 96, 128)]
        if mixed:
            engine.signed_txcomp_verify_device(d_items, n_items, d_blob, d_tio, d_tso, d_sch, d_keys, d_key_off, d_sigs,
                                               d_sig_off, txid, v_status, first_bad, sig_status, device=device, stream=s)
        else:
            engine.signed_txcomp_verify_ed25519_device(d_items, n_items, d_blob, d_tio, d_tso, d_keys[:nsig],
                                                       d_sigs[:nsig], txid, v_status, first_bad, sig_status,
                                                       device=device, stream=s)
        engine.txcomp_inputs_device(d_items, n_items, d_blob, d_tio, refs, tx_ref_off, tw_from, tw_until, gate,
                                    tx_status=v_status, ref_cap=ref_cap, device=device, stream=s)
        engine.commit_inputs_device(log_id, txid, d_caller, refs[:ref_cap], tx_ref_off, c_status, committed,
                                    ref_state, ref_by, tw_from, tw_until, now, tolerance, gate=gate, stream=s)
        if ecdsa_notary:
            engine.ecdsa_sign_keyed_device(d_key_id, txid, n_sigs, n_sig_len, s_status, gate=c_status, device=device,
                                           stream=s)
        elif rsa_notary:
            for sg_w, sl_w, st_w in rsa_out:  # a key of another class answers SIGN_UNKNOWN_KEY there
                engine.rsa_sign_keyed_device(d_key_id, txid, d_salts, sg_w, sl_w, st_w, gate=c_status, device=device,
                                             stream=s)
        else:
            engine.ed25519_sign_keyed_device(d_key_id, txid, n_sigs, s_status, gate=c_status, device=device, stream=s)
        status = torch.where(gate != 0, gate, c_status)
        # the one download
        out = [x.cpu().numpy() for x in (txid, status, committed, refs, tx_ref_off, ref_by, ref_state, n_sigs,
                                         s_status, v_status, n_sig_len)]
        if rsa_notary:
            rsa_host = [tuple(x.cpu().numpy() for x in o) for o in rsa_out]
    ids_a, status_a, committed_a, refs_a, off_a, by_a, state_a, sig_a, sst_a, verify_a, sig_len_a = out
    if detail is not None:
        detail.update(ids=ids_a, status=status_a, committed=committed_a, refs=refs_a[:ref_cap], tx_ref_off=off_a,
                      ref_state=state_a[:ref_cap], verify_status=verify_a)
    answers, rows = [], []
    for t in range(n):
        st, txid_t = int(status_a[t]), ids_a[t].tobytes()
        mine = [(refs_a[i, :32].tobytes(), int.from_bytes(refs_a[i, 32:].tobytes(), "little"))
                for i in range(int(off_a[t]), int(off_a[t + 1]))]
        if st not in _COMMIT_STATUSES or st == 18:
            # the id exists unless the tree or a component failed (mixed: a signature may fail in more ways)
            has_id = int(verify_a[t]) not in (6, 9) if mixed and st not in _COMMIT_STATUSES else int(verify_a[t]) in (OK, BAD_SIG)
            answers.append(NotaryError("TransactionInvalid", txid_t if has_id else None))
        elif st == _COMMIT_TIME_WINDOW_INVALID:
            answers.append(NotaryError("TimeWindowInvalid", txid_t))
        elif st == _COMMIT_CONFLICT:
            hist = {}
            for k, i in enumerate(range(int(off_a[t]), int(off_a[t + 1]))):
                if int(state_a[i]):
                    b = by_a[i]
                    hist.setdefault(mine[k], (b[:32].tobytes(), int.from_bytes(b[32:36].tobytes(), "little"),
                                              int.from_bytes(b[36:40].tobytes(), "little")))
            answers.append(NotaryError("Conflict", txid_t, hist))
        elif rsa_notary:
            mine_w = [o for o in rsa_host if int(o[2][t]) != _SIGN_UNKNOWN_KEY]
            if not mine_w:
                raise NoSuchElementException("no registered key %d" % key_id)
            answers.append(mine_w[0][0][t, :int(mine_w[0][1][t]) & 0xFFFF].tobytes())
        elif int(sst_a[t]) == _SIGN_UNKNOWN_KEY:
            raise NoSuchElementException("no registered key %d" % key_id)
        else:
            answers.append(sig_a[t, :int(sig_len_a[t])].tobytes() if ecdsa_notary else sig_a[t].tobytes())
        if committed_a[t]:
            last = {}
            for i, r in enumerate(mine):
                last[r] = (txid_t, i, int(callers[t]))
            rows.extend(last.items())
    return answers, rows


def validate_notary_signatures(engine, key_id: int, ids: Sequence[bytes], sigs: Sequence[bytes],
                               ecdsa: bool = False):
    """What a notary client does with the notary's answers (NotaryFlow.Client.call,
    NotaryFlow.kt:75-83: `check(sig.by in notaryParty.owningKey.keys); sig.verify(stx.id.bytes)`)
    for a batch of transactions notarised by one key: one Engine.verify_keyed_batch of sigs[t]
    over ids[t] against the verification key registered as `key_id` (the caller registered the
    notary identity's key, engine.vkey_add_ed25519, and sends here the signatures whose `by` is
    that key -- the membership check is a comparison of key bytes it has already made).
    ecdsa: the notary's key is an ECDSA key (engine.vkey_add_ecdsa, e.g. held in an HSM) and the
    signatures are DER: Engine.ecdsa_verify_keyed_batch instead.

    Returns one outcome per lane: None where the signature verifies, else the exception
    sig.verify throws (_lane_exception's mapping); an id that names no live key is a
    NoSuchElementException, as for the signer's registry."""
    if not ids:
        return []
    assert len(ids) == len(sigs)
    verify = engine.ecdsa_verify_keyed_batch if ecdsa else engine.verify_keyed_batch
    status, _ = verify([key_id] * len(ids), [bytes(s) for s in sigs], [bytes(i) for i in ids])
    out = []
    for st in status:
        st = int(st)
        if st == OK:
            out.append(None)
        elif st == _VERIFY_UNKNOWN_KEY:
            out.append(NoSuchElementException("no registered verification key %d" % key_id))
        else:
            out.append(_lane_exception(st))
    return out


def topological_sort(stxs: Sequence[SignedTx], ids: Sequence[bytes]) -> List[int]:
    """ResolveTransactionsFlow.topologicalSort (:40-66) over indices: dependencies
    before dependers, deterministic in input order. Iterative DFS (the Kotlin
    recursion, unrolled) so long chains do not hit Python's recursion limit."""
    forward = {}  # txhash -> dependent tx indices, insertion-ordered (LinkedHashSet)
    for t, stx in enumerate(stxs):
        for h in stx.inputs:
            forward.setdefault(h, {})[t] = None
    visited, result = set(), []
    for root in range(len(stxs)):
        if ids[root] in visited:
            continue
        visited.add(ids[root])
        stack = [(root, iter(forward.get(ids[root], ())))]
        while stack:
            t, it = stack[-1]
            nxt = next(it, None)
            if nxt is None:
                stack.pop()
                result.append(t)
            elif ids[nxt] not in visited:
                visited.add(ids[nxt])
                stack.append((nxt, iter(forward.get(ids[nxt], ()))))
    result.reverse()
    if len(result) != len(stxs):
        raise TransactionGraphException("Failed requirement.")
    return result


@dataclass
class Resolution:
    order: List[int]                    # topological order (indices into the input)
    recorded: List[int]                 # transactions that passed, in the order they were recorded
    failed: Optional[int] = None        # index of the transaction whose check threw
    error: Optional[Exception] = None   # what ResolveTransactionsFlow.call would throw
    outcomes: List[Outcome] = field(default_factory=list)


def resolve_transactions(engine, stxs: Sequence[SignedTx],
                         verify_contracts: Optional[Callable[[int, SignedTx], None]] = None) -> Resolution:
    """The verification loop of ResolveTransactionsFlow.call (:98-114) over already
    downloaded transactions: ids and signatures of all of them in one engine call,
    then, in topological order, the first exception stops the loop (earlier
    transactions stay recorded, as in the flow). verify_contracts(i, stx) stands
    in for transactionVerifierService.verify (contract logic is out of scope)."""
    outcomes = verify_signatures_batch(engine, stxs)
    res = Resolution(order=[], recorded=[], outcomes=outcomes)
    # A transaction without an id cannot even be sorted: the SignedTransaction
    # constructor (:37-39) or stx.id inside topologicalSort's visit() (:53-54)
    # throws before anything is recorded -- the first such one in input order.
    for t, o in enumerate(outcomes):
        if o.id is None:
            res.failed, res.error = t, o.error
            return res
    ids = [o.id for o in outcomes]
    try:
        res.order = topological_sort(stxs, ids)
    except TransactionGraphException as e:
        res.error = e
        return res
    for t in res.order:
        err = outcomes[t].error
        if err is None and verify_contracts is not None:
            try:
                verify_contracts(t, stxs[t])
            except Exception as e:  # noqa: BLE001 - the flow propagates whatever the verifier throws
                err = e
        if err is not None:
            res.failed, res.error = t, err
            return res
        res.recorded.append(t)
    return res
