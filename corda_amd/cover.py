"""Required-signer coverage: the wire form of include/cordahip.h's cordahip_cover
(tx.mustSign as post-order token streams over a shared key table) built from
resolve.CompositeKey trees or plain keys, and the context-free host evaluator
(cordahip_cover_eval_host).

Reference rule: SignedTransaction.getMissingSignatures (SignedTransaction.kt:102-108),
CompositeKey.isFulfilledBy (CompositeKey.kt:186-209).
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import check, lib

ED25519 = _lib.EDDSA_ED25519_SHA512


def _ptr(a) -> Optional[int]:
    return a.ctypes.data if a.size else None


class CoverArrays:
    """The arrays of one cordahip_cover (numpy, host) with its two outputs.

    tx_reqs[t] = [(tokens, allowed)] in tx.mustSign order, tokens = [(nchild, weight,
    threshold, key)] in post order; keys = [(scheme, key bytes)], the key table."""

    def __init__(self, tx_reqs: Sequence[Sequence[Tuple[Sequence[tuple], bool]]], keys: Sequence[Tuple[int, bytes]]):
        reqs = [r for per in tx_reqs for r in per]
        self.ntx, self.nreq, self.nckey = len(tx_reqs), len(reqs), len(keys)
        self.tx_req_off = np.zeros(self.ntx + 1, np.uint64)
        if tx_reqs:
            self.tx_req_off[1:] = np.cumsum([len(per) for per in tx_reqs], dtype=np.uint64)
        self.req_tok_off = np.zeros(self.nreq + 1, np.uint64)
        if reqs:
            self.req_tok_off[1:] = np.cumsum([len(toks) for toks, _ in reqs], dtype=np.uint64)
        flat = [tk for toks, _ in reqs for tk in toks]
        self.tok = np.zeros(len(flat), _lib.COVER_TOK_DTYPE)
        for name, col in zip(("nchild", "weight", "threshold", "key"), zip(*flat) if flat else ((),) * 4):
            self.tok[name] = np.asarray(col, np.uint64).astype(np.uint32)
        self.req_flags = np.asarray([1 if al else 0 for _, al in reqs], np.uint8)
        self.ckey_scheme = np.asarray([s for s, _ in keys], np.uint8)
        self.ckey_off = np.zeros(self.nckey + 1, np.uint64)
        if keys:
            self.ckey_off[1:] = np.cumsum([len(k) for _, k in keys], dtype=np.uint64)
        self.ckey = np.frombuffer(b"".join(k for _, k in keys), np.uint8).copy()
        self.req_status = np.full(self.nreq, 0xff, np.uint8)
        self.first_missing = np.full(max(self.ntx, 1), -99, np.int64)

    @classmethod
    def from_arrays(cls, tx_req_off, req_tok_off, tok, req_flags, ckey_scheme, ckey, ckey_off) -> "CoverArrays":
        """Over arrays that already have the wire form (a large synthetic batch)."""
        self = cls.__new__(cls)
        self.tx_req_off = np.ascontiguousarray(tx_req_off, np.uint64)
        self.req_tok_off = np.ascontiguousarray(req_tok_off, np.uint64)
        self.tok = np.ascontiguousarray(tok, _lib.COVER_TOK_DTYPE)
        self.req_flags = np.ascontiguousarray(req_flags, np.uint8)
        self.ckey_scheme = np.ascontiguousarray(ckey_scheme, np.uint8)
        self.ckey = np.ascontiguousarray(ckey, np.uint8).reshape(-1)
        self.ckey_off = np.ascontiguousarray(ckey_off, np.uint64)
        self.ntx, self.nreq, self.nckey = len(self.tx_req_off) - 1, len(self.req_tok_off) - 1, len(self.ckey_scheme)
        self.req_status = np.full(self.nreq, 0xff, np.uint8)
        self.first_missing = np.full(max(self.ntx, 1), -99, np.int64)
        return self

    @property
    def ntok(self) -> int:
        return len(self.tok)

    def struct(self) -> _lib.Cover:
        """The descriptor over the host arrays (which self keeps alive)."""
        return _lib.Cover(_ptr(self.tx_req_off), _ptr(self.req_tok_off), _ptr(self.tok), _ptr(self.req_flags),
                          _ptr(self.ckey_scheme), _ptr(self.ckey), _ptr(self.ckey_off), _ptr(self.req_status),
                          _ptr(self.first_missing), self.nreq, self.ntok, self.nckey, self.ckey.size)

    def to_device(self, device: int = 0):
        """(descriptor with DEVICE pointers for cordahip_tx_cover_device, the torch tensors behind
        it: keep them alive; 'req_status' and 'first_missing' receive the results)."""
        import torch
        dev = torch.device("cuda", device)

        def up(a, pad=16):  # never an empty allocation: a distinct, valid address per array
            b = np.zeros(max(a.nbytes, pad), np.uint8)
            b[:a.nbytes] = a.view(np.uint8).reshape(-1)
            return torch.from_numpy(b).to(dev)

        t = {name: up(getattr(self, name)) for name in ("tx_req_off", "req_tok_off", "tok", "req_flags", "ckey_scheme",
                                                        "ckey", "ckey_off", "req_status", "first_missing")}
        c = _lib.Cover(*[t[name].data_ptr() for name in ("tx_req_off", "req_tok_off", "tok", "req_flags",
                                                          "ckey_scheme", "ckey", "ckey_off", "req_status",
                                                          "first_missing")],
                       self.nreq, self.ntok, self.nckey, self.ckey.size)
        return c, t

    def from_device(self, tensors):
        """(req_status[nreq], first_missing[ntx]) of a finished cordahip_tx_cover_device as numpy."""
        rs = tensors["req_status"].cpu().numpy()[:self.nreq].copy()
        fm = tensors["first_missing"].cpu().numpy().view(np.int64)[:self.ntx].copy()
        return rs, fm


def _scheme_of(key: bytes, sigs: Iterable[tuple]) -> int:
    """A bare key's scheme: that of the transaction's signature with the same key
    bytes, if any (then byte equality is scheme-and-byte equality); else Ed25519
    for 32 bytes, and 0 -- no scheme, matching nothing -- otherwise."""
    for s, k, _ in sigs:
        if k == key:
            return s
    return ED25519 if len(key) == 32 else 0


def flatten_lists(must_sign: Sequence[Sequence], sigs: Optional[Sequence[Sequence[tuple]]] = None,
                  allowed_to_be_missing=()):
    """flatten's work as lists: (tx_reqs, keys) as CoverArrays takes them.

    must_sign[t] = tx.mustSign of transaction t: resolve.CompositeKey trees, (scheme, key
    bytes) pairs or bare key bytes (their scheme then comes from sigs[t], _scheme_of). Equal
    (scheme, key) leaves share one key-table entry across the batch. Trees are flattened as
    they are: an invalid one becomes a stream the library reports MALFORMED."""
    from .resolve import CompositeKey
    allowed = set(allowed_to_be_missing)
    table, keys = {}, []

    def leaf(node, weight, t):
        sk = (int(node[0]), bytes(node[1])) if isinstance(node, tuple) else \
            (_scheme_of(bytes(node), sigs[t] if sigs is not None else ()), bytes(node))
        if sk not in table:
            table[sk] = len(keys)
            keys.append(sk)
        return (0, weight, 0, table[sk])

    def walk(node, weight, t, out):  # post order, iteratively: deep chains must not hit the recursion limit
        work = [(node, weight, False)]
        while work:
            n, w, done = work.pop()
            if not isinstance(n, CompositeKey):
                out.append(leaf(n, w, t))
            elif done:
                out.append((len(n.children), w, n.threshold, 0))
            else:
                work.append((n, w, True))
                work.extend((ch, cw, False) for ch, cw in reversed(n.children))

    tx_reqs = []
    for t, per in enumerate(must_sign):
        reqs = []
        for k in per:
            toks: List[tuple] = []
            walk(k, 1, t, toks)
            reqs.append((toks, k in allowed))
        tx_reqs.append(reqs)
    return tx_reqs, keys


def flatten(must_sign: Sequence[Sequence], sigs: Optional[Sequence[Sequence[tuple]]] = None,
            allowed_to_be_missing=()) -> CoverArrays:
    """The cover arrays of a batch: flatten_lists(...) as a CoverArrays."""
    return CoverArrays(*flatten_lists(must_sign, sigs, allowed_to_be_missing))


def sig_key_arrays(sigs: Sequence[Sequence[tuple]]):
    """sigs[t] = [(scheme, key, ...)] -> (tx_sig_off, scheme, key blob, key_off) as numpy."""
    flat = [x for per in sigs for x in per]
    so = np.zeros(len(sigs) + 1, np.uint64)
    if sigs:
        so[1:] = np.cumsum([len(per) for per in sigs], dtype=np.uint64)
    sch = np.asarray([x[0] for x in flat], np.uint8)
    ko = np.zeros(len(flat) + 1, np.uint64)
    if flat:
        ko[1:] = np.cumsum([len(x[1]) for x in flat], dtype=np.uint64)
    kb = np.frombuffer(b"".join(bytes(x[1]) for x in flat), np.uint8).copy()
    return so, sch, kb, ko


def cover_eval_host(cover: CoverArrays, tx_status, sigs: Sequence[Sequence[tuple]]):
    """cordahip_cover_eval_host: the coverage rule on the host (no context, no device).
    tx_status[ntx] as the signature half left it; sigs[t] = [(scheme, key, ...)].
    Returns (tx_status, req_status, first_missing) -- new arrays; cover's outputs are filled too."""
    assert cover.ntx == len(sigs)
    return cover_eval_host_arrays(cover, tx_status, *sig_key_arrays(sigs))


def cover_eval_host_arrays(cover: CoverArrays, tx_status, so, sch, kb, ko):
    """cover_eval_host over the signature keys as arrays: tx_sig_off uint64[ntx + 1], scheme
    uint8[nsig], the key blob uint8 and key_off uint64[nsig + 1]."""
    n = cover.ntx
    st = np.array(tx_status, np.uint8, copy=True).reshape(-1)
    so, ko = np.ascontiguousarray(so, np.uint64), np.ascontiguousarray(ko, np.uint64)
    sch, kb = np.ascontiguousarray(sch, np.uint8), np.ascontiguousarray(kb, np.uint8).reshape(-1)
    assert len(st) == n == len(so) - 1
    c = cover.struct()
    check(lib().cordahip_cover_eval_host(ctypes.byref(c), n, _ptr(st), _ptr(so), _ptr(sch), _ptr(kb), _ptr(ko),
                                         len(sch), kb.size), "cordahip_cover_eval_host")
    return st, cover.req_status.copy(), cover.first_missing[:n].copy()
