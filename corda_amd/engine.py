"""Python handle on a libcordahip context (plumbing for tests and bench.py).

`Engine` owns one `cordahip_ctx`. Host batches go through the C-ABI's
generic CSR batch (`cordahip_sig_verify`, the `Crypto.isValid` batch
replacement) or the dense Ed25519 host path; device batches take torch
tensors that already live in HBM and run on the caller's HIP stream.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (EngineError, FilteredBuildBatch, FilteredTxBatch, SigBatch, SignedTxBatch, SignedTxcompBatch,
                   StreamBatch, TxcompBatch, TxidBatch, check, lib)


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


class Engine:
    def __init__(self, device_mask: int = 0):
        l = lib()
        self._ctx = ctypes.c_void_p()
        check(l.cordahip_init(device_mask, ctypes.byref(self._ctx)), "cordahip_init")
        self._signer_family = {}  # signer ids this engine registered: "ed25519", 2 or 3 (signer_family)

    def close(self):
        if self._ctx:
            lib().cordahip_shutdown(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def ctx(self):
        return self._ctx

    def device_count(self) -> int:
        return lib().cordahip_device_count(self._ctx)

    # ---- generic batch: Crypto.isValid per lane -------------------------------
    @staticmethod
    def _csr(items: Sequence[bytes]):
        off = np.zeros(len(items) + 1, dtype=np.uint64)
        if items:
            off[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
        blob = np.frombuffer(b"".join(items), dtype=np.uint8) if off[-1] else np.zeros(1, np.uint8)
        return np.ascontiguousarray(blob), off

    @staticmethod
    def _dev_args(stream, *tensors):
        """what a *_keyed_device wrapper hands the library: each tensor's device pointer (None for no
        tensor or one without elements) and the stream's handle (0: the null stream)"""
        ptrs = [(t.data_ptr() or None) if t is not None else None for t in tensors]
        return ptrs, (stream.cuda_stream if stream is not None else 0)

    def _run(self, name: str, b, submit: bool, res, keep):
        """the named host call on descriptor b, or its _submit: res(), or a Ticket whose wait() returns it"""
        if submit:
            t = ctypes.c_uint64()
            check(getattr(lib(), name + "_submit")(self._ctx, ctypes.byref(b), ctypes.byref(t)), name + "_submit")
            return Ticket(self, t.value, res, keep + (b,))
        check(getattr(lib(), name)(self._ctx, ctypes.byref(b)), name)
        return res()

    def _keyed_verify(self, name: str, key_ids, sigs, msgs, is_valid: bool, submit: bool):
        """a KeyedSigBatch of the lanes through the named call: (status[n], verdict) or a Ticket"""
        n = len(sigs)
        assert len(key_ids) == n and len(msgs) == n
        ids = np.ascontiguousarray(np.asarray(list(key_ids) or [0], dtype=np.uint32))
        sb, so = self._csr(list(sigs))
        mb, mo = self._csr(list(msgs))
        status = np.zeros(max(n, 1), dtype=np.uint8)
        verdict = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
        b = _lib.KeyedSigBatch(n, _ptr(ids), _ptr(sb), _ptr(so), _ptr(mb), _ptr(mo), _ptr(status), _ptr(verdict),
                               _lib.FLAG_IS_VALID if is_valid else 0, sb.size if n and so[n] else 0,
                               mb.size if n and mo[n] else 0)
        return self._run(name, b, submit, lambda: (status[:n], verdict), (ids, sb, so, mb, mo, status, verdict))

    def _keyed_sign(self, name: str, batch_type, row: int, with_len: bool, key_ids, msgs, gate, submit: bool):
        """a signing batch (SignBatch; EcdsaSignBatch with_len) through the named call: (sigs[n, row],
        [sig_len[n],] status[n]) or a Ticket"""
        n = len(msgs)
        assert len(key_ids) == n and (gate is None or len(gate) == n)
        ids = np.ascontiguousarray(np.asarray(list(key_ids) or [0], dtype=np.uint32))
        mb, mo = self._csr(list(msgs))
        g = None if gate is None else np.ascontiguousarray(np.asarray(list(gate) or [0], dtype=np.uint8))
        sig = np.zeros((max(n, 1), row), dtype=np.uint8)
        sl = [np.zeros(max(n, 1), dtype=np.uint8)] if with_len else []
        st = np.zeros(max(n, 1), dtype=np.uint8)
        b = batch_type(n, _ptr(ids), _ptr(mb), _ptr(mo), _ptr(g) if g is not None else None, _ptr(sig),
                       *[_ptr(a) for a in sl], _ptr(st), mb.size if n and mo[n] else 0)
        return self._run(name, b, submit, lambda: (sig[:n], *[a[:n] for a in sl], st[:n]), (ids, mb, mo, g, sig, sl, st))

    def verify_batch(self, schemes: Sequence[int], keys: Sequence[bytes], sigs: Sequence[bytes],
                     msgs: Sequence[bytes], async_: bool = False, is_valid: bool = False, rsa: bool = False):
        """Per-lane statuses for (scheme, key, sig, msg) tuples; returns (status, verdict).
        is_valid=False: Crypto.doVerify semantics (empty sig / clear data -> EMPTY);
        is_valid=True: Crypto.isValid semantics (no emptiness checks).
        rsa=True: RSA_SHA256 lanes (key = DER RSAPublicKey) are verified on the GPU
        (CORDAHIP_FLAG_RSA_ON_DEVICE); otherwise they are UNSUPPORTED."""
        n = len(keys)
        sch = np.ascontiguousarray(np.asarray(schemes, dtype=np.uint8))
        kb, ko = self._csr(list(keys))
        sb, so = self._csr(list(sigs))
        mb, mo = self._csr(list(msgs))
        status = np.zeros(max(n, 1), dtype=np.uint8)
        verdict = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
        b = SigBatch(n, _ptr(sch), _ptr(kb), _ptr(ko), _ptr(sb), _ptr(so), _ptr(mb), _ptr(mo),
                     _ptr(status), _ptr(verdict),
                     (_lib.FLAG_IS_VALID if is_valid else 0) | (_lib.FLAG_RSA_ON_DEVICE if rsa else 0),
                     kb.size, sb.size, mb.size)
        keep = (sch, kb, ko, sb, so, mb, mo, status, verdict, b)
        if async_:
            t = ctypes.c_uint64()
            check(lib().cordahip_sig_submit(self._ctx, ctypes.byref(b), ctypes.byref(t)), "cordahip_sig_submit")
            return Ticket(self, t.value, lambda: (status[:n], verdict), keep)
        check(lib().cordahip_sig_verify(self._ctx, ctypes.byref(b)), "cordahip_sig_verify")
        return status[:n], verdict

    # ---- dense Ed25519 host path ---------------------------------------------
    def ed25519_verify_host(self, keys: np.ndarray, sigs: np.ndarray, msgs: np.ndarray):
        keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 32)
        n = keys.shape[0]
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8).reshape(n, 64)
        msgs = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(n, -1)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        verdict = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
        check(lib().cordahip_ed25519_verify_host(self._ctx, _ptr(keys), _ptr(sigs), _ptr(msgs), msgs.shape[1], n,
                                                 _ptr(status), _ptr(verdict)), "cordahip_ed25519_verify_host")
        return status[:n], verdict

    # ---- device-resident paths (torch tensors in HBM) -------------------------
    def ed25519_verify_device(self, keys, sigs, msgs, status, verdict=None, device: int = 0, stream=None):
        n = keys.shape[0]
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_ed25519_verify_device(
            self._ctx, device, keys.data_ptr(), sigs.data_ptr(), msgs.data_ptr(), msgs.shape[1], n,
            status.data_ptr(), verdict.data_ptr() if verdict is not None else None, s),
            "cordahip_ed25519_verify_device")

    def ed25519_sign_device(self, seeds, msgs, pubs, sigs, device: int = 0, stream=None):
        n = seeds.shape[0]
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_ed25519_sign_device(self._ctx, device, seeds.data_ptr(), msgs.data_ptr(),
                                                 msgs.shape[1], n, pubs.data_ptr(), sigs.data_ptr(), s),
              "cordahip_ed25519_sign_device")

    # ---- Ed25519 signing with registered keys (Crypto.doSign per lane) -----------
    def signer_add_ed25519(self, seed: bytes):
        """cordahip_signer_add_ed25519: the 32-byte seed expanded on every device of the context.
        Returns (key_id, pub); the library keeps no host copy of the seed."""
        assert len(seed) == 32
        kid = ctypes.c_uint32()
        pub = ctypes.create_string_buffer(32)
        check(lib().cordahip_signer_add_ed25519(self._ctx, bytes(seed), ctypes.byref(kid), pub),
              "cordahip_signer_add_ed25519")
        self._signer_family[kid.value] = "ed25519"
        return kid.value, pub.raw

    def signer_remove(self, key_id: int):
        """cordahip_signer_remove: waits for the signing calls in flight, zeroes the key's record on
        every device; the id answers SIGN_UNKNOWN_KEY from then on."""
        check(lib().cordahip_signer_remove(self._ctx, key_id), "cordahip_signer_remove")
        self._signer_family.pop(int(key_id), None)

    def sign_batch(self, key_ids: Sequence[int], msgs: Sequence[bytes], gate=None, async_: bool = False):
        """cordahip_sign / cordahip_sign_submit: lane i signs msgs[i] with key key_ids[i] unless gate[i]
        is nonzero. Returns (sigs[n, 64], status[n]) -- zero rows where status is not OK -- or,
        async_, a Ticket whose wait() returns them."""
        return self._keyed_sign("cordahip_sign", _lib.SignBatch, 64, False, key_ids, msgs, gate, async_)

    def ed25519_sign_keyed_device(self, key_ids, msgs, sigs, status, gate=None, device: int = 0, stream=None):
        """cordahip_ed25519_sign_keyed_device over device tensors: key_ids int32 [n], msgs uint8
        [n, L], gate uint8 [n] or None (typically the tx_status an earlier call on `stream` wrote);
        outputs sigs uint8 [n, 64] and status uint8 [n]."""
        (k, m, g, sg, st), s = self._dev_args(stream, key_ids, msgs, gate, sigs, status)
        check(lib().cordahip_ed25519_sign_keyed_device(self._ctx, device, k, m, msgs.shape[1], key_ids.shape[0], g, sg,
                                                       st, s), "cordahip_ed25519_sign_keyed_device")

    # ---- ECDSA signing with registered keys (RFC 6979 nonces) ------------------------
    def signer_add_ecdsa(self, scheme: int, d: bytes):
        """cordahip_signer_add_ecdsa: the private scalar d (32 big-endian bytes) of scheme 2
        (secp256k1) or 3 (P-256) registered on every device of the context. Returns (key_id,
        key_status, pub): pub is Q = [d]G as 65 SEC1 bytes; (SIGNER_NO_ID, BAD_KEY, None) for d = 0 or
        d >= n (no slot taken). Ids share the Ed25519 signer's pool; signer_remove serves both."""
        assert len(d) == 32
        kid, st = ctypes.c_uint32(), ctypes.c_uint8()
        pub = ctypes.create_string_buffer(65)
        check(lib().cordahip_signer_add_ecdsa(self._ctx, scheme, bytes(d), ctypes.byref(kid), ctypes.byref(st), pub),
              "cordahip_signer_add_ecdsa")
        if st.value != 0:
            return kid.value, st.value, None
        self._signer_family[kid.value] = int(scheme)
        return kid.value, st.value, pub.raw

    def signer_family(self, key_id: int):
        """The family of a signer id this engine registered and has not removed: "ed25519", 2
        (ECDSA secp256k1), 3 (ECDSA P-256) or "rsa"; None for any other id."""
        return self._signer_family.get(int(key_id))

    def ecdsa_sign_batch(self, key_ids: Sequence[int], msgs: Sequence[bytes], gate=None, async_: bool = False):
        """cordahip_ecdsa_sign / cordahip_ecdsa_sign_submit: lane i signs msgs[i] with the ECDSA key
        key_ids[i] unless gate[i] is nonzero. Returns (sigs[n, 72], sig_len[n], status[n]) -- DER in
        zero-padded 72-byte slots, zero rows and length 0 where status is not OK -- or, async_, a
        Ticket whose wait() returns them."""
        return self._keyed_sign("cordahip_ecdsa_sign", _lib.EcdsaSignBatch, _lib.ECDSA_SIG_SLOT, True, key_ids, msgs,
                                gate, async_)

    def ecdsa_sign_keyed_device(self, key_ids, msgs, sigs, sig_len, status, gate=None, device: int = 0,
                                stream=None):
        """cordahip_ecdsa_sign_keyed_device over device tensors: key_ids int32 [n], msgs uint8 [n, L],
        gate uint8 [n] or None (typically the tx_status an earlier call on `stream` wrote); outputs
        sigs uint8 [n, 72], sig_len uint8 [n] and status uint8 [n]."""
        (k, m, g, sg, sl, st), s = self._dev_args(stream, key_ids, msgs, gate, sigs, sig_len, status)
        check(lib().cordahip_ecdsa_sign_keyed_device(self._ctx, device, k, m, msgs.shape[1], key_ids.shape[0], g, sg,
                                                     sl, st, s), "cordahip_ecdsa_sign_keyed_device")

    # ---- RSA_SHA256 signing with registered private keys (RSASSA-PSS, caller's salts) ------
    def signer_add_rsa(self, p: int, q: int, dp: int, dq: int, qinv: int, e: int):
        """cordahip_signer_add_rsa: the CRT components of an RSA private key (integers) and its public
        exponent registered on every device of the context. Returns (key_id, key_status, modulus):
        modulus is n = p q as k big-endian bytes; (SIGNER_NO_ID, UNSUPPORTED or BAD_KEY, None) for a
        key the GPU path declines or that is not one (no slot taken). An e that does not fit 32 bits
        cannot be expressed in the C call and is UNSUPPORTED here, as the verifier has it. Ids share the
        signer's pool; signer_remove serves all three families."""
        if not 0 <= e < 1 << 32:
            return _lib.SIGNER_NO_ID, _lib.UNSUPPORTED, None
        comp = [int(v).to_bytes(max((int(v).bit_length() + 7) // 8, 1), "big") for v in (p, q, dp, dq, qinv)]
        key = _lib.RsaPrivateKey(*comp, *[len(c) for c in comp], e)
        kid, st, ml = ctypes.c_uint32(), ctypes.c_uint8(), ctypes.c_uint32()
        mod = ctypes.create_string_buffer(512)
        check(lib().cordahip_signer_add_rsa(self._ctx, ctypes.byref(key), ctypes.byref(kid), ctypes.byref(st), mod,
                                            ctypes.byref(ml)), "cordahip_signer_add_rsa")
        if st.value != 0:
            return kid.value, st.value, None
        self._signer_family[kid.value] = "rsa"
        return kid.value, st.value, mod.raw[:ml.value]

    def rsa_sign_batch(self, key_ids: Sequence[int], msgs: Sequence[bytes], salts: Sequence[bytes], gate=None,
                       async_: bool = False):
        """cordahip_rsa_sign / cordahip_rsa_sign_submit: lane i signs msgs[i] with the RSA key key_ids[i]
        under the 32-byte salt salts[i] unless gate[i] is nonzero. Returns (sigs[n, 512], sig_len[n],
        status[n]) -- k bytes at the start of each slot, zero rows and length 0 where status is not OK
        -- or, async_, a Ticket whose wait() returns them."""
        n = len(msgs)
        assert len(key_ids) == n and len(salts) == n and (gate is None or len(gate) == n)
        assert all(len(x) == 32 for x in salts)
        ids = np.ascontiguousarray(np.asarray(list(key_ids) or [0], dtype=np.uint32))
        mb, mo = self._csr(list(msgs))
        sa = np.frombuffer(b"".join(bytes(x) for x in salts) or bytes(32), dtype=np.uint8).copy()
        g = None if gate is None else np.ascontiguousarray(np.asarray(list(gate) or [0], dtype=np.uint8))
        sig = np.zeros((max(n, 1), _lib.RSA_SIG_SLOT), dtype=np.uint8)
        sl = np.zeros(max(n, 1), dtype=np.uint16)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        b = _lib.RsaSignBatch(n, _ptr(ids), _ptr(mb), _ptr(mo), _ptr(g) if g is not None else None, _ptr(sa),
                              _ptr(sig), _ptr(sl), _ptr(st), mb.size if n and mo[n] else 0)
        return self._run("cordahip_rsa_sign", b, async_, lambda: (sig[:n], sl[:n], st[:n]),
                         (ids, mb, mo, sa, g, sig, sl, st))

    def rsa_sign_keyed_device(self, key_ids, msgs, salts, sigs, sig_len, status, gate=None, device: int = 0,
                              stream=None):
        """cordahip_rsa_sign_keyed_device over device tensors, one width class W = sigs.shape[1] // 4 per
        call: key_ids int32 [n], msgs uint8 [n, L], salts uint8 [n, 32], gate uint8 [n] or None
        (typically the tx_status an earlier call on `stream` wrote); outputs sigs uint8 [n, 4 W],
        sig_len int16 [n] and status uint8 [n]."""
        (k, m, sa, g, sg, sl, st), s = self._dev_args(stream, key_ids, msgs, salts, gate, sigs, sig_len, status)
        check(lib().cordahip_rsa_sign_keyed_device(self._ctx, device, k, m, msgs.shape[1], sa, sigs.shape[1] // 4,
                                                   key_ids.shape[0], g, sg, sl, st, s),
              "cordahip_rsa_sign_keyed_device")

    # ---- notary commit log (validateTimeWindow + commitInputStates per transaction) ----
    def commit_log_create(self, capacity_log2: int, device: int = 0, salt: Optional[bytes] = None) -> int:
        """cordahip_commit_log_create: an empty log of 2^capacity_log2 slots on `device`; salt: the
        16 bytes that key the slot index (None: drawn by the library). Returns the log id."""
        assert salt is None or len(salt) == 16
        lid = ctypes.c_uint32()
        check(lib().cordahip_commit_log_create(self._ctx, device, capacity_log2, salt, ctypes.byref(lid)),
              "cordahip_commit_log_create")
        return lid.value

    def commit_log_destroy(self, log_id: int):
        check(lib().cordahip_commit_log_destroy(self._ctx, log_id), "cordahip_commit_log_destroy")

    def commit_log_reserve(self, log_id: int, capacity_log2: int):
        """cordahip_commit_log_reserve: grow to 2^capacity_log2 slots and rehash on the device."""
        check(lib().cordahip_commit_log_reserve(self._ctx, log_id, capacity_log2), "cordahip_commit_log_reserve")

    def commit_log_stats(self, log_id: int):
        """(entries, capacity, next_seq) once every call enqueued on the log has finished."""
        e, c, s = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().cordahip_commit_log_stats(self._ctx, log_id, ctypes.byref(e), ctypes.byref(c), ctypes.byref(s)),
              "cordahip_commit_log_stats")
        return e.value, c.value, s.value

    @staticmethod
    def _state_refs(refs):
        a = np.zeros(max(len(refs), 1), dtype=_lib.STATE_REF_DTYPE)
        for i, (h, idx) in enumerate(refs):
            a[i]["txhash"] = np.frombuffer(bytes(h), np.uint8)
            a[i]["index"] = idx
        return a

    @staticmethod
    def _commit_rows(rows):
        a = np.zeros(max(len(rows), 1), dtype=_lib.COMMIT_ROW_DTYPE)
        for i, ((h, idx), (tid, pos, caller)) in enumerate(rows):
            a[i]["ref"]["txhash"] = np.frombuffer(bytes(h), np.uint8)
            a[i]["ref"]["index"] = idx
            a[i]["by"]["id"] = np.frombuffer(bytes(tid), np.uint8)
            a[i]["by"]["input_index"] = pos
            a[i]["by"]["caller"] = caller
        return a

    def commit_log_load(self, log_id: int, rows) -> int:
        """cordahip_commit_log_load: rows = [((txhash, index), (txid, input_index, caller))], the
        database's committed states at start-up. Returns how many were present already."""
        n = len(rows)
        a = self._commit_rows(rows)
        dup = ctypes.c_uint64()
        check(lib().cordahip_commit_log_load(self._ctx, log_id, a.ctypes.data if n else None, n, ctypes.byref(dup)),
              "cordahip_commit_log_load")
        return dup.value

    def commit_log_revoke(self, log_id: int, rows):
        """cordahip_commit_log_revoke: rows as commit_log_load takes them -- the rows of `committed`
        transactions whose database write failed. A row removes its ref's entry iff the stored
        (txid, input_index, caller) is exactly the row's. Returns (revoked, n_removed): a 0 / 1 per
        row, and the entries removed (equal rows count once)."""
        n = len(rows)
        a = self._commit_rows(rows)
        revoked = np.zeros(max(n, 1), dtype=np.uint8)
        removed = ctypes.c_uint64()
        check(lib().cordahip_commit_log_revoke(self._ctx, log_id, a.ctypes.data if n else None, n,
                                               revoked.ctypes.data if n else None, ctypes.byref(removed)),
              "cordahip_commit_log_revoke")
        return [int(x) for x in revoked[:n]], removed.value

    def commit_log_export(self, log_id: int, since_seq: int = 0):
        """cordahip_commit_log_export: [((txhash, index), (txid, input_index, caller), seq)] for every
        live entry whose sequence number is >= since_seq, in no particular order (a counting call
        first, then the call that fetches; both see the same log unless another thread changes it
        in between, in which case the rows that fitted are returned)."""
        total = ctypes.c_uint64()
        check(lib().cordahip_commit_log_export(self._ctx, log_id, since_seq, None, None, 0, ctypes.byref(total)),
              "cordahip_commit_log_export")
        cap = total.value
        if cap == 0:
            return []
        a = np.zeros(cap, dtype=_lib.COMMIT_ROW_DTYPE)
        seq = np.zeros(cap, dtype=np.uint64)
        check(lib().cordahip_commit_log_export(self._ctx, log_id, since_seq, a.ctypes.data, seq.ctypes.data, cap,
                                               ctypes.byref(total)), "cordahip_commit_log_export")
        return [((a[i]["ref"]["txhash"].tobytes(), int(a[i]["ref"]["index"])),
                 (a[i]["by"]["id"].tobytes(), int(a[i]["by"]["input_index"]), int(a[i]["by"]["caller"])), int(seq[i]))
                for i in range(min(cap, total.value))]

    def commit_log_lookup(self, log_id: int, refs):
        """cordahip_commit_log_lookup over refs = [(txhash, index)]: one entry per ref, None where
        absent, else the stored (txid, input_index, caller)."""
        n = len(refs)
        a = self._state_refs(refs)
        present = np.zeros(max(n, 1), dtype=np.uint8)
        by = np.zeros(max(n, 1), dtype=_lib.CONSUMING_TX_DTYPE)
        check(lib().cordahip_commit_log_lookup(self._ctx, log_id, a.ctypes.data if n else None, n,
                                               present.ctypes.data, by.ctypes.data), "cordahip_commit_log_lookup")
        return [(by[i]["id"].tobytes(), int(by[i]["input_index"]), int(by[i]["caller"])) if present[i] else None
                for i in range(n)]

    def commit_inputs(self, log_id: int, txs, now_ns: int = 0, tolerance_ns: int = 0, gate=None,
                      async_: bool = False):
        """cordahip_commit_inputs / _submit. txs[t] = (txid, caller, refs, window): txid 32 bytes,
        caller the requesting party's id, refs = [(txhash, index)] in input order, window None or
        (from_ns or None, until_ns or None) (sides beyond +-2^62 ns are saturated there). gate: a
        status per transaction (nonzero: skip), e.g. filtered_tx_verify's.
        Returns (tx_status[ntx], committed[ntx], ref_state, ref_by) with ref_state[t] / ref_by[t] one
        entry per input of transaction t (ref_by: None where absent, else (txid, input_index, caller));
        or, async_, a Ticket whose wait() returns them."""
        n = len(txs)
        assert gate is None or len(gate) == n
        flat = [r for tx in txs for r in tx[2]]
        nr = len(flat)
        txid = np.frombuffer(b"".join(bytes(tx[0]) for tx in txs) or bytes(32), dtype=np.uint8).copy()
        assert txid.size == max(n, 1) * 32
        caller = np.ascontiguousarray(np.asarray([tx[1] for tx in txs] or [0], dtype=np.uint32))
        refs = self._state_refs(flat)
        off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            off[1:] = np.cumsum([len(tx[2]) for tx in txs], dtype=np.uint64)
        fr = un = None
        if any(tx[3] is not None for tx in txs):
            def side(v):
                return _lib.TW_SIDE_ABSENT if v is None else max(-_lib.TW_SATURATE, min(_lib.TW_SATURATE, int(v)))
            fr = np.asarray([side(tx[3][0]) if tx[3] else _lib.TW_SIDE_ABSENT for tx in txs], dtype=np.int64)
            un = np.asarray([side(tx[3][1]) if tx[3] else _lib.TW_SIDE_ABSENT for tx in txs], dtype=np.int64)
        g = None if gate is None else np.ascontiguousarray(np.asarray(list(gate) or [0], dtype=np.uint8))
        st = np.zeros(max(n, 1), dtype=np.uint8)
        cm = np.zeros(max(n, 1), dtype=np.uint8)
        rs = np.zeros(max(nr, 1), dtype=np.uint8)
        rb = np.zeros(max(nr, 1), dtype=_lib.CONSUMING_TX_DTYPE)
        b = _lib.CommitBatch(n, _ptr(txid), _ptr(caller), refs.ctypes.data if nr else None, _ptr(off), nr,
                             _ptr(fr) if fr is not None else None, _ptr(un) if un is not None else None,
                             now_ns, tolerance_ns, _ptr(g) if g is not None else None, _ptr(st), _ptr(cm),
                             _ptr(rs), rb.ctypes.data)
        keep = (txid, caller, refs, off, fr, un, g, st, cm, rs, rb, b)

        def res():
            states, bys = [], []
            for t in range(n):
                a, z = int(off[t]), int(off[t + 1])
                states.append([int(x) for x in rs[a:z]])
                bys.append([(rb[i]["id"].tobytes(), int(rb[i]["input_index"]), int(rb[i]["caller"])) if rs[i] else None
                            for i in range(a, z)])
            return st[:n], cm[:n], states, bys

        if async_:
            t = ctypes.c_uint64()
            check(lib().cordahip_commit_inputs_submit(self._ctx, log_id, ctypes.byref(b), ctypes.byref(t)),
                  "cordahip_commit_inputs_submit")
            return Ticket(self, t.value, res, keep)
        check(lib().cordahip_commit_inputs(self._ctx, log_id, ctypes.byref(b)), "cordahip_commit_inputs")
        return res()

    def commit_inputs_submit(self, log_id: int, txs, now_ns: int = 0, tolerance_ns: int = 0, gate=None):
        """commit_inputs as a Ticket; tickets of one log commit in submit order."""
        return self.commit_inputs(log_id, txs, now_ns, tolerance_ns, gate, async_=True)

    def commit_inputs_device(self, log_id: int, txid, caller, refs, tx_ref_off, tx_status, committed, ref_state,
                             ref_by, tw_from=None, tw_until=None, now_ns: int = 0, tolerance_ns: int = 0, gate=None,
                             stream=None):
        """cordahip_commit_inputs_device over device tensors on the log's device: txid uint8 [ntx, 32],
        caller int32 [ntx], refs uint8 [n_refs, 36], tx_ref_off int64 [ntx + 1], tw_from / tw_until int64
        [ntx] or None, gate uint8 [ntx] or None (typically the tx_status an earlier call on `stream`
        wrote); outputs tx_status / committed uint8 [ntx], ref_state uint8 [n_refs], ref_by uint8
        [n_refs, 40]. tx_status can go straight in as ed25519_sign_keyed_device's gate."""
        s = stream.cuda_stream if stream is not None else 0
        p = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
        b = _lib.CommitBatch(txid.shape[0], p(txid), p(caller), p(refs), p(tx_ref_off), refs.shape[0], p(tw_from),
                             p(tw_until), now_ns, tolerance_ns, p(gate), p(tx_status), p(committed), p(ref_state),
                             p(ref_by))
        check(lib().cordahip_commit_inputs_device(self._ctx, log_id, ctypes.byref(b), s),
              "cordahip_commit_inputs_device")

    # ---- Ed25519 verification against registered keys (Crypto.doVerify / isValid per lane) ----
    def vkey_add_ed25519(self, key: bytes):
        """cordahip_vkey_add_ed25519: the 32 key bytes decoded and their window table built on every
        device of the context. Returns (key_id, key_status): (id, OK), or (VKEY_NO_ID, BAD_KEY) for bytes
        that are not a key (no slot taken). Ids are not the signer's ids."""
        assert len(key) == 32
        kid, st = ctypes.c_uint32(), ctypes.c_uint8()
        check(lib().cordahip_vkey_add_ed25519(self._ctx, bytes(key), ctypes.byref(kid), ctypes.byref(st)),
              "cordahip_vkey_add_ed25519")
        return kid.value, st.value

    def vkey_remove(self, key_id: int):
        """cordahip_vkey_remove: waits for the keyed calls in flight, clears the key's record on every
        device; the id answers VERIFY_UNKNOWN_KEY from then on."""
        check(lib().cordahip_vkey_remove(self._ctx, key_id), "cordahip_vkey_remove")

    def vkey_set_routing(self, on: bool):
        """cordahip_vkey_set_routing: on, every Ed25519 batch (generic, signed-tx, dense, stream) sends
        the lanes whose 32 key bytes equal a registered key's canonical encoding to the keyed verifier,
        on the GPU; statuses are those of the unrouted call. Off (the default): nothing changes."""
        check(lib().cordahip_vkey_set_routing(self._ctx, 1 if on else 0), "cordahip_vkey_set_routing")

    def vkey_route_stats(self, device: int = 0):
        """cordahip_vkey_route_stats: (keyed_lanes, generic_lanes) that routed enqueues on `device` have
        sent each way since init; waits for the routed work already enqueued there."""
        k, g = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().cordahip_vkey_route_stats(self._ctx, device, ctypes.byref(k), ctypes.byref(g)),
              "cordahip_vkey_route_stats")
        return k.value, g.value

    def vkey_set_routing_ecdsa(self, on: bool):
        """cordahip_vkey_set_routing_ecdsa: on, every ECDSA batch (generic, signed-tx, dense, stream) sends
        the lanes whose scheme and key bytes are a SEC1 encoding (04 || X || Y or (02 | Y & 1) || X) of a
        registered ECDSA key's point to the keyed verifier, on the GPU; statuses are those of the unrouted
        call. Off (the default): nothing changes. Ed25519 routing is a switch of its own."""
        check(lib().cordahip_vkey_set_routing_ecdsa(self._ctx, 1 if on else 0), "cordahip_vkey_set_routing_ecdsa")

    def vkey_route_stats_ecdsa(self, device: int = 0):
        """cordahip_vkey_route_stats_ecdsa: (keyed_lanes, generic_lanes) that routed ECDSA enqueues on
        `device` have sent each way since init; waits for the routed work already enqueued there."""
        k, g = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().cordahip_vkey_route_stats_ecdsa(self._ctx, device, ctypes.byref(k), ctypes.byref(g)),
              "cordahip_vkey_route_stats_ecdsa")
        return k.value, g.value

    def vkey_set_routing_rsa(self, on: bool):
        """cordahip_vkey_set_routing_rsa: on, every generic RSA launch (the dense device call, the RSA section
        of a generic batch with FLAG_RSA_ON_DEVICE) sends the rows whose width class, exponent and modulus
        words are a registered RSA key's to the keyed exponentiation, on the GPU; statuses are those of the
        unrouted call. Off (the default): nothing changes. The other families' switches are their own."""
        check(lib().cordahip_vkey_set_routing_rsa(self._ctx, 1 if on else 0), "cordahip_vkey_set_routing_rsa")

    def vkey_set_routing_device(self, on: bool):
        """cordahip_vkey_set_routing_device: on, the mixed device-resident calls (sig_verify_device,
        signed_tx_verify_device, signed_txcomp_verify_device, and resolve.notarise_transactions over them)
        let each family's packed rows follow that family's routing switch above and its live keys;
        statuses are those of the unrouted call. Off (the default): those calls ignore the switches."""
        check(lib().cordahip_vkey_set_routing_device(self._ctx, 1 if on else 0), "cordahip_vkey_set_routing_device")

    def set_rsa_on_device(self, on: bool):
        """cordahip_set_rsa_on_device: on, the signed-transaction host calls (signed_tx_verify, tx_submit,
        their covered and component forms) verify RSA_SHA256 signatures on the GPU, each over its
        transaction's id under doVerify rules, instead of answering UNSUPPORTED. Off: the default."""
        check(lib().cordahip_set_rsa_on_device(self._ctx, 1 if on else 0), "cordahip_set_rsa_on_device")

    def vkey_route_stats_rsa(self, device: int = 0):
        """cordahip_vkey_route_stats_rsa: (keyed_rows, generic_rows) that routed RSA enqueues on `device`
        have matched and not matched since init; waits for the routed work already enqueued there."""
        k, g = ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().cordahip_vkey_route_stats_rsa(self._ctx, device, ctypes.byref(k), ctypes.byref(g)),
              "cordahip_vkey_route_stats_rsa")
        return k.value, g.value

    def verify_keyed_batch(self, key_ids: Sequence[int], sigs: Sequence[bytes], msgs: Sequence[bytes],
                           is_valid: bool = False, async_: bool = False):
        """cordahip_verify_keyed / cordahip_verify_keyed_submit: lane i checks sigs[i] over msgs[i] against
        the registered key key_ids[i]. Returns (status[n], verdict) -- or, async_, a Ticket whose wait()
        returns them. is_valid as in verify_batch."""
        return self._keyed_verify("cordahip_verify_keyed", key_ids, sigs, msgs, is_valid, async_)

    # ---- ECDSA verification against registered keys (the same registry: one pool of ids) ----
    def vkey_add_ecdsa(self, scheme: int, key: bytes):
        """cordahip_vkey_add_ecdsa: the SEC1 key bytes (scheme 2: secp256k1, 3: P-256) decoded and their
        window table built on every device of the context. Returns (key_id, key_status): (id, OK), or
        (VKEY_NO_ID, BAD_KEY) for bytes that are not a key of the curve (no slot taken). vkey_remove
        removes the key."""
        kid, st = ctypes.c_uint32(), ctypes.c_uint8()
        check(lib().cordahip_vkey_add_ecdsa(self._ctx, scheme, bytes(key), len(key), ctypes.byref(kid),
                                            ctypes.byref(st)), "cordahip_vkey_add_ecdsa")
        return kid.value, st.value

    def ecdsa_verify_keyed_batch(self, key_ids: Sequence[int], sigs: Sequence[bytes], msgs: Sequence[bytes],
                                 is_valid: bool = False, submit: bool = False):
        """cordahip_ecdsa_verify_keyed / cordahip_ecdsa_verify_keyed_submit: lane i checks the DER signature
        sigs[i] over msgs[i] against the registered ECDSA key key_ids[i]. Returns (status[n], verdict) -- or,
        submit, a Ticket whose wait() returns them. is_valid as in verify_batch."""
        return self._keyed_verify("cordahip_ecdsa_verify_keyed", key_ids, sigs, msgs, is_valid, submit)

    def ecdsa_verify_keyed_device(self, key_ids, sigs, sig_len, msgs, status, verdict=None, device: int = 0,
                                  stream=None):
        """cordahip_ecdsa_verify_keyed_device over device tensors: key_ids int32 [n], sigs uint8 [n, 72],
        sig_len uint8 [n], msgs uint8 [n, L]; outputs status uint8 [n] and verdict int64 [(n + 63) // 64]
        or None."""
        (k, sg, sl, m, st, v), s = self._dev_args(stream, key_ids, sigs, sig_len, msgs, status, verdict)
        check(lib().cordahip_ecdsa_verify_keyed_device(self._ctx, device, k, sg, sl, m, msgs.shape[1],
                                                       key_ids.shape[0], st, v, s),
              "cordahip_ecdsa_verify_keyed_device")

    # ---- RSA_SHA256 verification against registered keys (the same registry: one pool of ids) ----
    def vkey_add_rsa(self, der: bytes):
        """cordahip_vkey_add_rsa: the SPKI BIT STRING payload (DER RSAPublicKey) decoded as a generic lane's
        key is, and its record (n', n, K = R^e mod n) copied to every device of the context. Returns
        (key_id, key_status): (id, OK), or (VKEY_NO_ID, BAD_KEY / UNSUPPORTED) for bytes that do not decode
        or a key the GPU path declines (no slot taken). vkey_remove removes the key."""
        kid, st = ctypes.c_uint32(), ctypes.c_uint8()
        check(lib().cordahip_vkey_add_rsa(self._ctx, bytes(der), len(der), ctypes.byref(kid), ctypes.byref(st)),
              "cordahip_vkey_add_rsa")
        return kid.value, st.value

    def rsa_verify_keyed_batch(self, key_ids: Sequence[int], sigs: Sequence[bytes], msgs: Sequence[bytes],
                               is_valid: bool = False, async_: bool = False):
        """cordahip_rsa_verify_keyed / cordahip_rsa_verify_keyed_submit: lane i checks the RSASSA-PSS
        signature sigs[i] over msgs[i] against the registered RSA key key_ids[i]. Returns (status[n], verdict)
        -- or, async_, a Ticket whose wait() returns them. is_valid as in verify_batch."""
        return self._keyed_verify("cordahip_rsa_verify_keyed", key_ids, sigs, msgs, is_valid, async_)

    def rsa_verify_keyed_device(self, key_ids, sigs, sig_len, msgs, status, verdict=None, device: int = 0,
                                stream=None):
        """cordahip_rsa_verify_keyed_device over device tensors, one width class W = sigs.shape[1] // 4 per
        call: key_ids int32 [n], sigs uint8 [n, 4 W] big-endian, sig_len int16 [n], msgs uint8 [n, L];
        outputs status uint8 [n] and verdict int64 [(n + 63) // 64] or None; doVerify statuses."""
        (k, sg, sl, m, st, v), s = self._dev_args(stream, key_ids, sigs, sig_len, msgs, status, verdict)
        check(lib().cordahip_rsa_verify_keyed_device(self._ctx, device, k, sg, sl, m, msgs.shape[1],
                                                     sigs.shape[1] // 4, key_ids.shape[0], st, v, s),
              "cordahip_rsa_verify_keyed_device")

    def rsa_public_op_keyed_device(self, key_ids, inp, out, device: int = 0, stream=None):
        """out = inp^e mod n of the registered RSA key key_ids[i] per row. Device tensors: key_ids int32 [n],
        inp / out [n, W] int32 (little-endian words, W = 64, 96 or 128: the call's width class). A row whose
        id names no live RSA key of that class, or with inp >= n, comes back zero."""
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_rsa_public_op_keyed_device(self._ctx, device, key_ids.data_ptr(), inp.data_ptr(),
                                                        inp.shape[1], inp.shape[0], out.data_ptr(), s),
              "cordahip_rsa_public_op_keyed_device")

    def ed25519_verify_keyed_device(self, key_ids, sigs, msgs, status, verdict=None, device: int = 0, stream=None):
        """cordahip_ed25519_verify_keyed_device over device tensors: key_ids int32 [n], sigs uint8 [n, 64],
        msgs uint8 [n, L]; outputs status uint8 [n] and verdict int64 [(n + 63) // 64] or None."""
        (k, sg, m, st, v), s = self._dev_args(stream, key_ids, sigs, msgs, status, verdict)
        check(lib().cordahip_ed25519_verify_keyed_device(self._ctx, device, k, sg, m, msgs.shape[1], key_ids.shape[0],
                                                         st, v, s), "cordahip_ed25519_verify_keyed_device")

    def ecdsa_sign_device(self, scheme, seeds, msgs, keys, key_len, sigs, sig_len, device: int = 0, stream=None):
        """Device tensors: scheme[n] u8 (2/3), seeds[n,32], msgs[n,L] -> keys[n,65], key_len[n], sigs[n,72], sig_len[n]."""
        n = seeds.shape[0]
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_ecdsa_sign_device(self._ctx, device, scheme.data_ptr(), seeds.data_ptr(), msgs.data_ptr(),
                                               msgs.shape[1], n, keys.data_ptr(), key_len.data_ptr(), sigs.data_ptr(),
                                               sig_len.data_ptr(), s), "cordahip_ecdsa_sign_device")

    # ---- transactions: WireTransaction.id and SignedTransaction verification ---
    def _tx_arrays(self, txs: Sequence[Sequence[bytes]]):
        leaves = [leaf for tx in txs for leaf in tx]
        lb, lo = self._csr(leaves)
        to = np.zeros(len(txs) + 1, dtype=np.uint64)
        if txs:
            to[1:] = np.cumsum([len(tx) for tx in txs], dtype=np.uint64)
        txid = np.zeros((max(len(txs), 1), 32), dtype=np.uint8)
        st = np.zeros(max(len(txs), 1), dtype=np.uint8)
        b = TxidBatch(len(txs), _ptr(lb), _ptr(lo), _ptr(to), _ptr(txid), _ptr(st), len(leaves), lb.size)
        return b, (lb, lo, to, txid, st)

    def tx_ids(self, txs: Sequence[Sequence[bytes]], async_: bool = False):
        """txs: per transaction, the serialised components (leaf preimages). Returns (ids[ntx,32], status[ntx])
        (or a Ticket whose wait() returns them)."""
        b, keep = self._tx_arrays(txs)
        res = lambda: (keep[3][:len(txs)], keep[4][:len(txs)])  # noqa: E731
        if async_:
            t = ctypes.c_uint64()
            check(lib().cordahip_txid_submit(self._ctx, ctypes.byref(b), ctypes.byref(t)), "cordahip_txid_submit")
            return Ticket(self, t.value, res, (b, keep))
        check(lib().cordahip_tx_ids(self._ctx, ctypes.byref(b)), "cordahip_tx_ids")
        return res()

    def signed_tx_verify(self, txs: Sequence[Sequence[bytes]], sigs: Sequence[Sequence[tuple]],
                         async_: bool = False, cover=None):
        """sigs[t] = [(scheme, key, sig), ...] in list order. Returns (ids, tx_status, first_bad, sig_status)
        (or, async_, a Ticket from cordahip_tx_submit whose wait() returns them). cover: see
        signed_tx_verify_covered."""
        b, keep = self._tx_arrays(txs)
        flat = [x for per in sigs for x in per]
        so = np.zeros(len(txs) + 1, dtype=np.uint64)
        if txs:
            so[1:] = np.cumsum([len(per) for per in sigs], dtype=np.uint64)
        sch = np.ascontiguousarray(np.asarray([x[0] for x in flat] or [0], dtype=np.uint8))
        kb, ko = self._csr([x[1] for x in flat])
        sb, sgo = self._csr([x[2] for x in flat])
        sst = np.zeros(max(len(flat), 1), dtype=np.uint8)
        fb = np.zeros(max(len(txs), 1), dtype=np.int64)
        sbatch = SignedTxBatch(b, _ptr(so), _ptr(sch), _ptr(kb), _ptr(ko), _ptr(sb), _ptr(sgo), _ptr(sst), _ptr(fb),
                               len(flat), kb.size, sb.size)
        n = len(txs)
        res = lambda: (keep[3][:n], keep[4][:n], fb[:n], sst[:len(flat)])  # noqa: E731
        hold = (keep, so, sch, kb, ko, sb, sgo, sst, fb, sbatch)
        if cover is not None:
            assert cover.ntx == n
            cs = cover.struct()
            res = lambda: (keep[3][:n], keep[4][:n], fb[:n], sst[:len(flat)],  # noqa: E731
                           cover.req_status, cover.first_missing[:n])
            if async_:
                t = ctypes.c_uint64()
                check(lib().cordahip_tx_submit_covered(self._ctx, ctypes.byref(sbatch), ctypes.byref(cs),
                                                       ctypes.byref(t)), "cordahip_tx_submit_covered")
                return Ticket(self, t.value, res, (hold, cover))  # the descriptor was copied at submit
            check(lib().cordahip_signed_tx_verify_covered(self._ctx, ctypes.byref(sbatch), ctypes.byref(cs)),
                  "cordahip_signed_tx_verify_covered")
            return res()
        if async_:
            t = ctypes.c_uint64()
            check(lib().cordahip_tx_submit(self._ctx, ctypes.byref(sbatch), ctypes.byref(t)), "cordahip_tx_submit")
            return Ticket(self, t.value, res, hold)
        check(lib().cordahip_signed_tx_verify(self._ctx, ctypes.byref(sbatch)), "cordahip_signed_tx_verify")
        return res()

    def signed_tx_verify_covered(self, txs, sigs, cover, async_: bool = False):
        """cordahip_signed_tx_verify_covered / cordahip_tx_submit_covered: signed_tx_verify followed by
        the required-signer coverage of `cover` (a cover.CoverArrays, e.g. cover.flatten(must_sign,
        sigs)) -- the whole of verifySignatures. Returns (ids, tx_status, first_bad, sig_status,
        req_status, first_missing); the last two are cover's own output arrays."""
        return self.signed_tx_verify(txs, sigs, async_=async_, cover=cover)

    def signed_txcomp_verify_covered(self, txs, sigs, cover, async_: bool = False):
        """cordahip_signed_txcomp_verify_covered / cordahip_txcomp_submit_covered: as
        signed_tx_verify_covered, over components (signed_txcomp_verify's txs)."""
        return self.signed_txcomp_verify(txs, sigs, async_=async_, cover=cover)

    def tx_cover_device(self, ntx: int, tx_status, tx_sig_off, sig_key, cover_struct, sig_scheme=None,
                        sig_key_off=None, device: int = 0, stream=None):
        """cordahip_tx_cover_device: the coverage kernel on `stream`, after a *_ed25519_device
        signed-tx call that left tx_status / tx_sig_off / its keys (sig_key) in HBM. cover_struct: a
        _lib.Cover with device pointers (CoverArrays.to_device). sig_scheme None: all Ed25519;
        sig_key_off None: sig_key holds dense 32-byte rows."""
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_tx_cover_device(
            self._ctx, device, ntx, tx_status.data_ptr(), tx_sig_off.data_ptr(),
            sig_scheme.data_ptr() if sig_scheme is not None else None, sig_key.data_ptr(),
            sig_key_off.data_ptr() if sig_key_off is not None else None, ctypes.byref(cover_struct), s),
            "cordahip_tx_cover_device")

    def signed_txcomp_verify(self, txs, sigs, async_: bool = False, cover=None):
        """cordahip_signed_txcomp_verify / cordahip_txcomp_submit: txs[t] = the transaction's components
        as (kind, value, class_id) tuples (_lib.kryo_pack's form, availableComponents order) -- the GPU
        writes their leaves; sigs as in signed_tx_verify. Returns (ids, tx_status, first_bad, sig_status)."""
        comps = [c for tx in txs for c in tx]
        blob, items, has = _lib.kryo_pack(comps)
        items = items.copy()
        items["data"] = np.where(has, items["data"], 0)  # offsets into the payload
        tio = np.zeros(len(txs) + 1, dtype=np.uint64)
        if txs:
            tio[1:] = np.cumsum([len(tx) for tx in txs], dtype=np.uint64)
        return self.signed_txcomp_verify_arrays(np.ascontiguousarray(blob), items, tio, sigs, async_=async_,
                                                cover=cover)

    def signed_txcomp_verify_arrays(self, payload, items, tx_item_off, sigs, async_: bool = False,
                                    pinned_out: bool = False, cover=None):
        """The array form: payload uint8, items KRYO_ITEM_DTYPE whose `data` are offsets into payload,
        tx_item_off uint64[ntx + 1]; sigs[t] = [(scheme, key, sig), ...]. pinned_out: txid and
        tx_status in page-locked memory (the library's kernels then store them through their
        device mapping, as for a JVM's pinned direct buffers)."""
        n = len(tx_item_off) - 1
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        items = np.ascontiguousarray(items)
        tio = np.ascontiguousarray(tx_item_off, dtype=np.uint64)
        pins = ()
        if pinned_out:
            import torch
            pins = (torch.zeros((max(n, 1), 32), dtype=torch.uint8).pin_memory(),
                    torch.zeros(max(n, 1), dtype=torch.uint8).pin_memory())
            txid, st = pins[0].numpy(), pins[1].numpy()
        else:
            txid = np.zeros((max(n, 1), 32), dtype=np.uint8)
            st = np.zeros(max(n, 1), dtype=np.uint8)
        tb = TxcompBatch(n, _ptr(items) if len(items) else None, _ptr(tio), _ptr(payload) if payload.size else None,
                         payload.size, _ptr(txid), _ptr(st), len(items))
        flat = [x for per in sigs for x in per]
        so = np.zeros(n + 1, dtype=np.uint64)
        if n:
            so[1:] = np.cumsum([len(per) for per in sigs], dtype=np.uint64)
        sch = np.ascontiguousarray(np.asarray([x[0] for x in flat] or [0], dtype=np.uint8))
        kb, ko = self._csr([x[1] for x in flat])
        sb, sgo = self._csr([x[2] for x in flat])
        sst = np.zeros(max(len(flat), 1), dtype=np.uint8)
        fb = np.zeros(max(n, 1), dtype=np.int64)
        sbatch = SignedTxcompBatch(tb, _ptr(so), _ptr(sch), _ptr(kb), _ptr(ko), _ptr(sb), _ptr(sgo), _ptr(sst),
                                   _ptr(fb), len(flat), kb.size, sb.size)
        res = lambda: (txid[:n], st[:n], fb[:n], sst[:len(flat)])  # noqa: E731
        keep = (payload, items, tio, txid, st, so, sch, kb, ko, sb, sgo, sst, fb, tb, sbatch, pins)
        if cover is not None:  # the _covered forms: results grow by (req_status, first_missing)
            assert cover.ntx == n
            cs = cover.struct()
            res = lambda: (txid[:n], st[:n], fb[:n], sst[:len(flat)],  # noqa: E731
                           cover.req_status, cover.first_missing[:n])
            if async_:
                t = ctypes.c_uint64()
                check(lib().cordahip_txcomp_submit_covered(self._ctx, ctypes.byref(sbatch), ctypes.byref(cs),
                                                           ctypes.byref(t)), "cordahip_txcomp_submit_covered")
                return Ticket(self, t.value, res, (keep, cover))
            check(lib().cordahip_signed_txcomp_verify_covered(self._ctx, ctypes.byref(sbatch), ctypes.byref(cs)),
                  "cordahip_signed_txcomp_verify_covered")
            return res()
        if async_:
            t = ctypes.c_uint64()
            check(lib().cordahip_txcomp_submit(self._ctx, ctypes.byref(sbatch), ctypes.byref(t)),
                  "cordahip_txcomp_submit")
            return Ticket(self, t.value, res, keep)
        check(lib().cordahip_signed_txcomp_verify(self._ctx, ctypes.byref(sbatch)), "cordahip_signed_txcomp_verify")
        return res()

    def signed_tx_verify_ed25519_device(self, leaf_bytes, leaf_off, tx_leaf_off, tx_sig_off, keys, sigs,
                                        txid, tx_status, first_bad, sig_status, device: int = 0, stream=None):
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_signed_tx_verify_ed25519_device(
            self._ctx, device, leaf_bytes.data_ptr(), leaf_off.data_ptr(), leaf_off.shape[0] - 1,
            tx_leaf_off.data_ptr(), tx_leaf_off.shape[0] - 1, tx_sig_off.data_ptr(), keys.data_ptr(),
            sigs.data_ptr(), keys.shape[0], txid.data_ptr(), tx_status.data_ptr(), first_bad.data_ptr(),
            sig_status.data_ptr(), s), "cordahip_signed_tx_verify_ed25519_device")

    def signed_txcomp_verify_ed25519_device(self, items, n_items: int, payload, tx_item_off, tx_sig_off, keys, sigs,
                                            txid, tx_status, first_bad, sig_status, group: int = 1, device: int = 0,
                                            stream=None):
        """cordahip_signed_txcomp_verify_ed25519_device: items (device tensor of n_items
        cordahip_kryo_item records whose `data` are offsets into payload), payload (uint8 device
        tensor), tx_item_off / tx_sig_off (int64 [ntx + 1]), keys [nsig, 32], sigs [nsig, 64];
        outputs as in signed_tx_verify_ed25519_device."""
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_signed_txcomp_verify_ed25519_device(
            self._ctx, device, items.data_ptr(), n_items, group, payload.data_ptr() if payload.numel() else None,
            payload.numel(), tx_item_off.data_ptr(), tx_item_off.shape[0] - 1, tx_sig_off.data_ptr(),
            keys.data_ptr(), sigs.data_ptr(), keys.shape[0], txid.data_ptr(), tx_status.data_ptr(),
            first_bad.data_ptr(), sig_status.data_ptr(), s), "cordahip_signed_txcomp_verify_ed25519_device")

    def signed_tx_verify_device(self, leaf_bytes, leaf_off, tx_leaf_off, tx_sig_off, scheme, key, key_off, sig,
                                sig_off, txid, tx_status, first_bad, sig_status, device: int = 0, stream=None):
        """cordahip_signed_tx_verify_device (K23): signed_tx_verify_ed25519_device with signatures of
        any scheme -- scheme uint8 [nsig], key / sig uint8 byte buffers, key_off / sig_off int64
        [nsig + 1]; RSA lanes follow set_rsa_on_device."""
        s = stream.cuda_stream if stream is not None else 0
        p = lambda x: x.data_ptr() if x.numel() else None  # noqa: E731
        check(lib().cordahip_signed_tx_verify_device(
            self._ctx, device, p(leaf_bytes), leaf_off.data_ptr(), leaf_off.shape[0] - 1, tx_leaf_off.data_ptr(),
            tx_leaf_off.shape[0] - 1, tx_sig_off.data_ptr(), p(scheme), p(key), key_off.data_ptr(), key.numel(),
            p(sig), sig_off.data_ptr(), sig.numel(), scheme.numel(), txid.data_ptr(), tx_status.data_ptr(),
            first_bad.data_ptr(), p(sig_status), s), "cordahip_signed_tx_verify_device")

    def signed_txcomp_verify_device(self, items, n_items: int, payload, tx_item_off, tx_sig_off, scheme, key, key_off,
                                    sig, sig_off, txid, tx_status, first_bad, sig_status, group: int = 1,
                                    device: int = 0, stream=None):
        """cordahip_signed_txcomp_verify_device (K23): signed_txcomp_verify_ed25519_device with the
        signatures as signed_tx_verify_device takes them."""
        s = stream.cuda_stream if stream is not None else 0
        p = lambda x: x.data_ptr() if x.numel() else None  # noqa: E731
        check(lib().cordahip_signed_txcomp_verify_device(
            self._ctx, device, items.data_ptr(), n_items, group, p(payload), payload.numel(), tx_item_off.data_ptr(),
            tx_item_off.shape[0] - 1, tx_sig_off.data_ptr(), p(scheme), p(key), key_off.data_ptr(), key.numel(),
            p(sig), sig_off.data_ptr(), sig.numel(), scheme.numel(), txid.data_ptr(), tx_status.data_ptr(),
            first_bad.data_ptr(), p(sig_status), s), "cordahip_signed_txcomp_verify_device")

    def txcomp_inputs_device(self, items, n_items: int, payload, tx_item_off, refs, tx_ref_off, tw_from, tw_until,
                             gate, tx_status=None, ref_cap: Optional[int] = None, device: int = 0, stream=None):
        """cordahip_txcomp_inputs_device (K22): the STATE_REF and TIME_WINDOW items of the component
        batch signed_txcomp_verify_ed25519_device takes (items, n_items, payload, tx_item_off) as the
        device rows commit_inputs_device takes. Outputs: refs uint8 [ref_cap, 36] (ref_cap: its rows
        unless given), tx_ref_off int64 [ntx + 1], tw_from / tw_until int64 [ntx], gate uint8 [ntx]
        (tx_status -- uint8 [ntx] or None, typically the verify call's -- where that is nonzero, else
        TX_BAD_COMPONENT for a transaction whose items or range were flagged, else 0)."""
        s = stream.cuda_stream if stream is not None else 0
        p = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
        check(lib().cordahip_txcomp_inputs_device(
            self._ctx, device, p(items), n_items, p(payload), payload.numel(), p(tx_item_off),
            tx_item_off.shape[0] - 1, p(tx_status), p(refs), refs.shape[0] if ref_cap is None else ref_cap,
            p(tx_ref_off), p(tw_from), p(tw_until), p(gate), s), "cordahip_txcomp_inputs_device")

    def device_mem(self, device: int = 0):
        """cordahip_device_mem: (bytes the library holds on the device's GPU, their peak, the budget)"""
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        check(lib().cordahip_device_mem(self._ctx, device, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
              "cordahip_device_mem")
        return a.value, b.value, c.value

    def trim(self):
        """cordahip_trim: release every device's grow-only buffers now"""
        check(lib().cordahip_trim(self._ctx), "cordahip_trim")

    def kryo_encode_device(self, items, n: int, out, off, status, group: int = 1, device: int = 0, stream=None):
        """cordahip_kryo_encode_device: leaf preimages of n components on the GPU. items: a
        device tensor holding n cordahip_kryo_item records (_lib.KRYO_ITEM_DTYPE) whose data
        pointers are device addresses; out: uint8 device tensor (its size is the cap); off:
        n + 1 int64; status: n uint8 (0 written, 1 invalid item, 2 beyond cap)."""
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_kryo_encode_device(self._ctx, device, items.data_ptr(), n, group,
                                                out.data_ptr() if out is not None else None,
                                                out.numel() if out is not None else 0, off.data_ptr(),
                                                status.data_ptr(), s), "cordahip_kryo_encode_device")

    def kryo_encode_packed_device(self, blob, items, has, group: int = 1, cap=None, device: int = 0, stream=None):
        """_lib.kryo_pack output (payload blob, items with blob offsets, has-payload mask) encoded on
        the GPU: the blob and the rebased items go to the device, then cordahip_kryo_encode_device.
        cap None: sized by a first pass. Synchronous (returns host-visible results): (leaves uint8
        device tensor, off int64 device tensor [n + 1], status uint8 device tensor [n])."""
        import contextlib

        import torch
        dev = torch.device("cuda", device)
        # the copies and zero fills are ordered before the encoder on `stream`
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            d_blob = torch.from_numpy(np.ascontiguousarray(blob)).to(dev)
            a = np.array(items, copy=True)
            a["data"] = np.where(has, a["data"] + np.uint64(d_blob.data_ptr()), 0)
            d_items = torch.from_numpy(a.view(np.uint8)).to(dev)
            n = len(a)
            off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            status = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        if cap is None:
            self.kryo_encode_device(d_items, n, None, off, status, group, device, stream)
            torch.cuda.synchronize(dev)
            cap = int(off[n])
        out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        self.kryo_encode_device(d_items, n, out, off, status, group, device, stream)
        torch.cuda.synchronize(dev)
        return out[:cap], off, status[:n]

    def ecdsa_verify_device(self, scheme, keys, key_len, sigs, sig_len, msgs, status, verdict=None, device: int = 0,
                            stream=None):
        """Dense mixed secp256k1/P-256 batch in HBM: keys [n,65] + key_len, DER sigs [n,72] + sig_len."""
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_ecdsa_verify_device(
            self._ctx, device, scheme.data_ptr(), keys.data_ptr(), key_len.data_ptr(), sigs.data_ptr(),
            sig_len.data_ptr(), msgs.data_ptr(), msgs.shape[1], scheme.shape[0], status.data_ptr(),
            verdict.data_ptr() if verdict is not None else None, s), "cordahip_ecdsa_verify_device")

    def rsa_public_op_device(self, mod, exp, inp, out, device: int = 0, stream=None):
        """out = inp^exp mod mod per row. Device tensors: mod / inp / out [n, W] int32 (little-endian
        words, W = 64, 96 or 128), exp [n] int32. Needs an odd modulus, exp >= 1 and inp < mod;
        a row that breaks this comes back zero."""
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_rsa_public_op_device(self._ctx, device, mod.data_ptr(), exp.data_ptr(), inp.data_ptr(),
                                                  mod.shape[1], mod.shape[0], out.data_ptr(), s),
              "cordahip_rsa_public_op_device")

    def rsa_pss_verify_device(self, mod, exp, sigs, sig_len, msgs, status, verdict=None, device: int = 0,
                              stream=None):
        """Dense RSASSA-PSS batch in HBM: mod [n, W] int32 little-endian words, exp [n] int32,
        sigs [n, 4 W] uint8 big-endian + sig_len [n] int16, msgs [n, L] uint8; doVerify statuses."""
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_rsa_pss_verify_device(
            self._ctx, device, mod.data_ptr(), exp.data_ptr(), sigs.data_ptr(), sig_len.data_ptr(),
            msgs.data_ptr() if msgs.shape[1] else None, msgs.shape[1], mod.shape[1], mod.shape[0],
            status.data_ptr(), verdict.data_ptr() if verdict is not None else None, s),
            "cordahip_rsa_pss_verify_device")

    def sig_verify_device(self, scheme, key, key_off, sig, sig_off, msgs, status, verdict=None, msg_row=None,
                          is_valid: bool = False, rsa_on_device: bool = False, device: int = 0, stream=None,
                          key_bytes=None, sig_bytes=None):
        """The generic mixed-scheme batch resident in HBM (K23): scheme [n] uint8, key / sig uint8 byte
        buffers with key_off / sig_off [n + 1] int64 CSR offsets, msgs [rows, L] uint8, msg_row [n] int32
        (None: lane i signs row i). Classified, packed and verified on the GPU; statuses in lane order
        (BAD_RANGE for a lane whose ranges or message row are out of bounds). key_bytes / sig_bytes:
        the buffers' declared sizes (default: the tensors')."""
        s = stream.cuda_stream if stream is not None else 0
        flags = (_lib.FLAG_IS_VALID if is_valid else 0) | (_lib.FLAG_RSA_ON_DEVICE if rsa_on_device else 0)
        kb = key.numel() if key_bytes is None else key_bytes
        sb = sig.numel() if sig_bytes is None else sig_bytes
        check(lib().cordahip_sig_verify_device(
            self._ctx, device, scheme.data_ptr() if scheme.numel() else None, key.data_ptr() if key.numel() else None,
            key_off.data_ptr(), kb, sig.data_ptr() if sig.numel() else None, sig_off.data_ptr(), sb,
            msgs.data_ptr() if msgs.numel() else None, msgs.shape[1], msg_row.data_ptr() if msg_row is not None else None,
            msgs.shape[0], scheme.numel(), flags, status.data_ptr() if status.numel() else None,
            verdict.data_ptr() if verdict is not None else None, s),
            "cordahip_sig_verify_device")

    # ---- FilteredTransaction.verify / PartialMerkleTree.verify ----------------
    def filtered_tx_verify(self, ftxs, async_: bool = False):
        """ftxs[t] = (leaves: [bytes], tokens: [(tok, hash32 or None)], root: bytes32), tokens being the
        post-order stream of the PartialMerkleTree (oracle/partial_merkle.py tokens()). Returns tx_status."""
        leaves = [leaf for f in ftxs for leaf in f[0]]
        lb, lo = self._csr(leaves)
        to = np.zeros(len(ftxs) + 1, dtype=np.uint64)
        ko = np.zeros(len(ftxs) + 1, dtype=np.uint64)
        if ftxs:
            to[1:] = np.cumsum([len(f[0]) for f in ftxs], dtype=np.uint64)
            ko[1:] = np.cumsum([len(f[1]) for f in ftxs], dtype=np.uint64)
        toks = [t for f in ftxs for t in f[1]]
        tok = np.ascontiguousarray(np.array([t[0] for t in toks] or [0], dtype=np.uint8))
        th = np.frombuffer(b"".join((t[1] or bytes(32)) for t in toks) or bytes(32), dtype=np.uint8).copy()
        root = np.frombuffer(b"".join(f[2] for f in ftxs) or bytes(32), dtype=np.uint8).copy()
        st = np.zeros(max(len(ftxs), 1), dtype=np.uint8)
        b = FilteredTxBatch(len(ftxs), _ptr(lb), _ptr(lo), _ptr(to), _ptr(tok), _ptr(th), _ptr(ko), _ptr(root),
                            _ptr(st), len(leaves), lb.size, len(toks))
        if async_:
            t = ctypes.c_uint64()
            check(lib().cordahip_filtered_tx_submit(self._ctx, ctypes.byref(b), ctypes.byref(t)),
                  "cordahip_filtered_tx_submit")
            return Ticket(self, t.value, lambda: st[:len(ftxs)], (lb, lo, to, tok, th, ko, root, st, b))
        check(lib().cordahip_filtered_tx_verify(self._ctx, ctypes.byref(b)), "cordahip_filtered_tx_verify")
        return st[:len(ftxs)]

    # ---- notary tear-offs from typed refs and windows (K21 + K6, then K16) ------
    def _tearoff_arrays(self, tearoffs, leaf_hash: bool):
        """tearoffs[t] = (refs: [(txhash, index)], window: None or (from, until) with a side None or
        (epochSecond, nano), tokens: [(tok, hash32 or None)], root: bytes32) as the arrays of a
        cordahip_notary_tearoff_batch; returns (batch, keep, off, st, lh)."""
        n = len(tearoffs)
        flat = [r for f in tearoffs for r in f[0]]
        nr = len(flat)
        refs = self._state_refs(flat)
        off = np.zeros(n + 1, dtype=np.uint64)
        ko = np.zeros(n + 1, dtype=np.uint64)
        if n:
            off[1:] = np.cumsum([len(f[0]) for f in tearoffs], dtype=np.uint64)
            ko[1:] = np.cumsum([len(f[2]) for f in tearoffs], dtype=np.uint64)
        fl = fs = fn = us = un = None
        nwin = sum(1 for f in tearoffs if f[1] is not None)
        if nwin:
            fl = np.zeros(n, dtype=np.uint8)
            fs, us = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
            fn, un = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
            for t, f in enumerate(tearoffs):
                if f[1] is None:
                    continue
                a, z = f[1]
                fl[t] = _lib.TW_PRESENT | (a is not None) | ((z is not None) << 1)
                if a is not None:
                    fs[t], fn[t] = a
                if z is not None:
                    us[t], un[t] = z
        toks = [t for f in tearoffs for t in f[2]]
        tok = np.ascontiguousarray(np.array([t[0] for t in toks] or [0], dtype=np.uint8))
        th = np.frombuffer(b"".join((t[1] or bytes(32)) for t in toks) or bytes(32), dtype=np.uint8).copy()
        root = np.frombuffer(b"".join(bytes(f[3]) for f in tearoffs) or bytes(32), dtype=np.uint8).copy()
        st = np.zeros(max(n, 1), dtype=np.uint8)
        lh = np.zeros((max(nr + nwin, 1), 32), dtype=np.uint8) if leaf_hash else None
        p = lambda x: _ptr(x) if x is not None else None  # noqa: E731
        b = _lib.NotaryTearoffBatch(n, refs.ctypes.data if nr else None, _ptr(off), nr, p(fl), p(fs), p(fn), p(us),
                                    p(un), _ptr(tok), _ptr(th), _ptr(ko), len(toks), _ptr(root), _ptr(st), p(lh))
        return b, (refs, off, ko, fl, fs, fn, us, un, tok, th, root, st, lh, b), off, st, lh

    def notary_tearoff_verify(self, tearoffs, leaf_hash: bool = False, async_: bool = False):
        """cordahip_notary_tearoff_verify / _submit: FilteredTransaction.verify of tear-offs given as
        typed components (tearoffs as _tearoff_arrays takes them), their StateRef / TimeWindow leaves
        hashed on the GPU. Returns tx_status[ntx] -- with leaf_hash, (tx_status, hashes [leaves, 32])
        in availableComponents order -- or, async_, a Ticket whose wait() returns that."""
        n = len(tearoffs)
        b, keep, _, st, lh = self._tearoff_arrays(tearoffs, leaf_hash)
        nl = sum(len(f[0]) + (f[1] is not None) for f in tearoffs)
        res = (lambda: (st[:n], lh[:nl])) if leaf_hash else (lambda: st[:n])
        if async_:
            t = ctypes.c_uint64()
            check(lib().cordahip_notary_tearoff_submit(self._ctx, ctypes.byref(b), ctypes.byref(t)),
                  "cordahip_notary_tearoff_submit")
            return Ticket(self, t.value, res, keep)
        check(lib().cordahip_notary_tearoff_verify(self._ctx, ctypes.byref(b)), "cordahip_notary_tearoff_verify")
        return res()

    def notary_tearoff_commit(self, log_id: int, tearoffs, callers, now_ns: int = 0, tolerance_ns: int = 0,
                              gate=None, async_: bool = False):
        """cordahip_notary_tearoff_commit / _commit_submit: verify the typed tear-offs and commit the
        refs of those that verify, on the log's device, gated by `gate` (nonzero: skip) as well.
        Returns (tx_status, committed, ref_state, ref_by) shaped as commit_inputs returns them;
        tx_status is the verify status where that is not OK, else the commit's."""
        n = len(tearoffs)
        assert len(callers) == n and (gate is None or len(gate) == n)
        b, keep, off, st, _ = self._tearoff_arrays(tearoffs, False)
        nr = int(off[n])
        caller = np.ascontiguousarray(np.asarray(list(callers) or [0], dtype=np.uint32))
        g = None if gate is None else np.ascontiguousarray(np.asarray(list(gate) or [0], dtype=np.uint8))
        cm = np.zeros(max(n, 1), dtype=np.uint8)
        rs = np.zeros(max(nr, 1), dtype=np.uint8)
        rb = np.zeros(max(nr, 1), dtype=_lib.CONSUMING_TX_DTYPE)
        args = (self._ctx, log_id, ctypes.byref(b), _ptr(caller), now_ns, tolerance_ns,
                _ptr(g) if g is not None else None, _ptr(cm), _ptr(rs), rb.ctypes.data)

        def res():
            states, bys = [], []
            for t in range(n):
                a, z = int(off[t]), int(off[t + 1])
                states.append([int(x) for x in rs[a:z]])
                bys.append([(rb[i]["id"].tobytes(), int(rb[i]["input_index"]), int(rb[i]["caller"])) if rs[i] else None
                            for i in range(a, z)])
            return st[:n], cm[:n], states, bys

        if async_:
            t = ctypes.c_uint64()
            check(lib().cordahip_notary_tearoff_commit_submit(*args, ctypes.byref(t)),
                  "cordahip_notary_tearoff_commit_submit")
            return Ticket(self, t.value, res, keep + (caller, g, cm, rs, rb))
        check(lib().cordahip_notary_tearoff_commit(*args), "cordahip_notary_tearoff_commit")
        return res()

    def notary_tearoff_device(self, refs, tx_ref_off, tok, tok_hash, tx_tok_off, root, tx_status, tw_from, tw_until,
                              tw_flags=None, tw_from_s=None, tw_from_nano=None, tw_until_s=None, tw_until_nano=None,
                              leaf_hash=None, device: int = 0, stream=None):
        """cordahip_notary_tearoff_device over device tensors: refs uint8 [n_refs, 36], tx_ref_off /
        tx_tok_off int64 [ntx + 1], tok uint8 [ntok], tok_hash uint8 [ntok, 32], root uint8 [ntx, 32],
        the window rows (uint8 / int64 / int32 [ntx], all or none); outputs tx_status uint8 [ntx],
        tw_from / tw_until int64 [ntx], leaf_hash uint8 [leaves, 32] or None."""
        s = stream.cuda_stream if stream is not None else 0
        p = lambda x: x.data_ptr() if x is not None and x.numel() else None  # noqa: E731
        b = _lib.NotaryTearoffBatch(root.shape[0], p(refs), p(tx_ref_off), refs.shape[0], p(tw_flags), p(tw_from_s),
                                    p(tw_from_nano), p(tw_until_s), p(tw_until_nano), p(tok), p(tok_hash),
                                    p(tx_tok_off), tok.shape[0], p(root), p(tx_status), p(leaf_hash))
        check(lib().cordahip_notary_tearoff_device(self._ctx, device, ctypes.byref(b), p(tw_from), p(tw_until), s),
              "cordahip_notary_tearoff_device")

    # ---- FilteredTransaction build / PartialMerkleTree.build -------------------
    def filtered_tx_build(self, txs, async_: bool = False):
        """txs[t] = (leaves: [bytes], include: [bool]), one include flag per leaf (the filter predicate's
        verdict on that component). The token slots are sized by the bound (_lib.pmt_slot_bound). Returns
        (ids[ntx,32], status[ntx], tokens) with tokens[t] = [(tok, hash32 or None), ...], the form
        filtered_tx_verify takes (empty for a non-OK transaction); or, async_, a Ticket whose wait()
        returns them."""
        n = len(txs)
        leaves = [leaf for tx in txs for leaf in tx[0]]
        lb, lo = self._csr(leaves)
        inc = np.ascontiguousarray(np.array([1 if f else 0 for tx in txs for f in tx[1]] or [0], dtype=np.uint8))
        assert all(len(tx[0]) == len(tx[1]) for tx in txs)
        to = np.zeros(n + 1, dtype=np.uint64)
        ko = np.zeros(n + 1, dtype=np.uint64)
        if n:
            to[1:] = np.cumsum([len(tx[0]) for tx in txs], dtype=np.uint64)
            ko[1:] = np.cumsum([_lib.pmt_slot_bound(len(tx[0])) for tx in txs], dtype=np.uint64)
        ntok = int(ko[n])
        tok = np.zeros(max(ntok, 1), dtype=np.uint8)
        th = np.zeros((max(ntok, 1), 32), dtype=np.uint8)
        txid = np.zeros((max(n, 1), 32), dtype=np.uint8)
        cnt = np.zeros(max(n, 1), dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        b = FilteredBuildBatch(n, _ptr(lb), _ptr(lo), _ptr(to), _ptr(inc), _ptr(ko), _ptr(txid), _ptr(tok), _ptr(th),
                               _ptr(cnt), _ptr(st), len(leaves), lb.size, ntok)

        def res():
            out = []
            for t in range(n):
                k0 = int(ko[t])
                out.append([(int(tok[k]), None if tok[k] == 2 else th[k].tobytes())
                            for k in range(k0, k0 + int(cnt[t]))])
            return txid[:n], st[:n], out

        if async_:
            t = ctypes.c_uint64()
            check(lib().cordahip_filtered_tx_build_submit(self._ctx, ctypes.byref(b), ctypes.byref(t)),
                  "cordahip_filtered_tx_build_submit")
            return Ticket(self, t.value, res, (lb, lo, to, inc, ko, txid, tok, th, cnt, st, b))
        check(lib().cordahip_filtered_tx_build(self._ctx, ctypes.byref(b)), "cordahip_filtered_tx_build")
        return res()

    def filtered_tx_build_device(self, leaf_bytes, leaf_off, tx_leaf_off, include, tx_tok_off, txid, tok, tok_hash,
                                 tx_ntok, tx_status, device: int = 0, stream=None):
        """cordahip_filtered_tx_build_device over device tensors: leaf_bytes uint8, leaf_off int64
        [nleaves + 1], tx_leaf_off / tx_tok_off int64 [ntx + 1], include uint8 [nleaves]; outputs
        txid [ntx, 32], tok [ntok], tok_hash [ntok, 32] uint8, tx_ntok int64 [ntx], tx_status uint8 [ntx]."""
        s = stream.cuda_stream if stream is not None else 0
        check(lib().cordahip_filtered_tx_build_device(
            self._ctx, device, leaf_bytes.data_ptr(), leaf_off.data_ptr(), leaf_off.shape[0] - 1,
            tx_leaf_off.data_ptr(), tx_leaf_off.shape[0] - 1, include.data_ptr(), tx_tok_off.data_ptr(),
            tok.shape[0], txid.data_ptr(), tok.data_ptr(), tok_hash.data_ptr(), tx_ntok.data_ptr(),
            tx_status.data_ptr(), s), "cordahip_filtered_tx_build_device")

    # ---- C5: streaming mixed-scheme drain (host, ideally pinned, memory) -------
    def stream_verify(self, ed, ec):
        """ed = (keys[n,32], sigs[n,64], msgs[n,L], status[n]) and ec = (scheme[n], keys[n,65],
        key_len[n], sigs[n,72], sig_len[n], msgs[n,L], status[n]): host arrays (numpy or CPU torch
        tensors; pin them for overlapped copies). Statuses are written in place."""
        def p(x):
            return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data

        ek, es, em, est = ed
        sc, ck, ckl, cs, csl, cm, cst = ec
        b = StreamBatch(ek.shape[0], p(ek), p(es), p(em), em.shape[1] if ek.shape[0] else 0, p(est),
                        sc.shape[0], p(sc), p(ck), p(ckl), p(cs), p(csl), p(cm), cm.shape[1] if sc.shape[0] else 0,
                        p(cst))
        check(lib().cordahip_stream_verify(self._ctx, ctypes.byref(b)), "cordahip_stream_verify")

    def last_kernel_ms(self, device: int = 0) -> float:
        return lib().cordahip_last_kernel_ms(self._ctx, device)


class Ticket:
    """A submitted batch (cordahip_*_submit). wait() releases the ticket and returns the
    batch's results; poll() only reports completion. `keep` pins the host buffers."""

    def __init__(self, eng: Engine, ticket: int, result, keep):
        self.eng, self.ticket, self._result, self._keep = eng, ticket, result, keep
        self._waited = False

    def __del__(self):
        # a ticket dropped without wait(): the pool may still be writing into the
        # buffers self._keep pins, so wait for it before they can be freed
        if not getattr(self, "_waited", True) and self.eng.ctx:
            lib().cordahip_wait(self.eng.ctx, self.ticket, -1)

    def poll(self) -> bool:
        r = lib().cordahip_poll(self.eng.ctx, self.ticket)
        if r < 0:
            raise EngineError(r, "cordahip_poll")
        return r == 1

    def wait(self, timeout_ns: int = -1):
        rc = lib().cordahip_wait(self.eng.ctx, self.ticket, timeout_ns)
        if rc != _lib.ERR_TIMEOUT:
            self._waited = True  # released by the library (successfully or not)
        check(rc, "cordahip_wait")
        return self._result()
