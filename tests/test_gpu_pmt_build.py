"""FilteredTransaction build on the GPU (cordahip_filtered_tx_build, K3 + K10)
against tests/golden/pmt_build_vectors.json (the oracle's PartialMerkleTree.build):
ids, statuses, token counts and tokens byte for byte; the built tear-offs
through cordahip_filtered_tx_verify (K6); the ticketed and device-resident
forms; the slot guard of the device-resident call and the host forms' validation."""
import ctypes
import json
import os

import numpy as np
import pytest

from corda_amd import _lib
from corda_amd._lib import lib

pytestmark = pytest.mark.gpu
INVALID = -1
GUARD = 48  # guard entries before tx_tok_off[0] and after tx_tok_off[ntx]


@pytest.fixture(scope="module")
def cases():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pmt_build_vectors.json")
    out = []
    for c in json.load(open(path))["cases"]:
        out.append(dict(c, leaves=[bytes.fromhex(x) for x in c["leaves"]], root=bytes.fromhex(c["root"]),
                        tokens=[(t, bytes.fromhex(h) if h else None) for t, h in c["tokens"]]))
    return out


class Arrays:
    """The batch's arrays with exact-bound slots (a transaction in `short` gets one token less),
    guard entries around the slots, and recognisable fill in every output."""

    def __init__(self, cases, short=()):
        self.n = n = len(cases)
        leaves = [x for c in cases for x in c["leaves"]]
        self.nleaves = len(leaves)
        self.lo = np.zeros(len(leaves) + 1, np.uint64)
        self.lo[1:] = np.cumsum([len(x) for x in leaves])
        self.lb = np.frombuffer(b"".join(leaves) or b"\0", np.uint8).copy()
        self.tlo = np.zeros(n + 1, np.uint64)
        self.tlo[1:] = np.cumsum([len(c["leaves"]) for c in cases])
        self.inc = np.array([f for c in cases for f in c["include"]] or [0], np.uint8)
        self.tko = np.zeros(n + 1, np.uint64)
        self.tko[0] = GUARD
        self.tko[1:] = GUARD + np.cumsum([_lib.pmt_slot_bound(len(c["leaves"])) - (1 if t in short else 0)
                                          for t, c in enumerate(cases)])
        self.ntok = int(self.tko[n]) + GUARD
        self.tok = np.full(self.ntok, 0xA5, np.uint8)
        self.th = np.full((self.ntok, 32), 0xA5, np.uint8)
        self.txid = np.full((n, 32), 0xA5, np.uint8)
        self.cnt = np.full(n, 0xA5A5A5A5, np.uint64)
        self.st = np.full(n, 0xA5, np.uint8)

    def batch(self, tko=None, ntok=None):
        p = lambda a: a.ctypes.data  # noqa: E731
        return _lib.FilteredBuildBatch(self.n, p(self.lb), p(self.lo), p(self.tlo), p(self.inc),
                                       p(self.tko if tko is None else tko), p(self.txid), p(self.tok), p(self.th),
                                       p(self.cnt), p(self.st), self.nleaves, self.lb.size,
                                       self.ntok if ntok is None else ntok)

    def outputs(self):
        return [x.copy() for x in (self.txid, self.tok, self.th, self.cnt, self.st)]

    def tokens(self, t):
        k0 = int(self.tko[t])
        return [(int(self.tok[k]), None if self.tok[k] == 2 else self.th[k].tobytes())
                for k in range(k0, k0 + int(self.cnt[t]))]


def check_against_golden(a, cases, skip=()):
    for t, c in enumerate(cases):
        if t in skip:
            continue
        assert a.st[t] == c["status"], c["name"]
        if c["leaves"]:
            assert a.txid[t].tobytes() == c["root"], c["name"]
        else:
            assert not a.txid[t].any()
        assert a.cnt[t] == len(c["tokens"]), c["name"]
        assert a.tokens(t) == c["tokens"], c["name"]
    for arr in (a.tok, a.th):  # nothing outside [tx_tok_off[0], tx_tok_off[ntx]) is written
        assert (arr[:GUARD] == 0xA5).all() and (arr[int(a.tko[a.n]):] == 0xA5).all()


def test_goldens_one_batch(engine, cases):
    a = Arrays(cases)
    assert lib().cordahip_filtered_tx_build(engine.ctx, ctypes.byref(a.batch())) == 0
    check_against_golden(a, cases)
    assert {int(x) for x in a.st} == {0, 6, 12}
    ids, st = engine.tx_ids([c["leaves"] for c in cases])
    assert np.array_equal(ids, a.txid) and np.array_equal(st == 6, a.st == 6)
    # the Python mirror sizes the slots itself and returns the same
    ids2, st2, toks2 = engine.filtered_tx_build([(c["leaves"], c["include"]) for c in cases])
    assert np.array_equal(ids2, a.txid) and np.array_equal(st2, a.st)
    assert toks2 == [c["tokens"] for c in cases]


def test_round_trip_through_verify(engine, cases):
    built = engine.filtered_tx_build([(c["leaves"], c["include"]) for c in cases])
    ok = [t for t, c in enumerate(cases) if c["status"] == 0]
    ftxs = [([x for x, f in zip(cases[t]["leaves"], cases[t]["include"]) if f], built[2][t], bytes(built[0][t]))
            for t in ok]
    want = np.array([0 if any(cases[t]["include"]) else 6 for t in ok], np.uint8)
    assert (want == 0).sum() > 30 and (want == 6).sum() >= 2
    assert np.array_equal(engine.filtered_tx_verify(ftxs), want)
    # one bit of one token hash flipped in every tree: the comparison sees the tokens
    bad = []
    for i, (leaves, toks, root) in enumerate(ftxs):
        toks = list(toks)
        k = [j for j, (tk, _) in enumerate(toks) if tk != 2][i % sum(tk != 2 for tk, _ in toks)]
        h = bytearray(toks[k][1])
        h[i % 32] ^= 1 << (i % 8)
        toks[k] = (toks[k][0], bytes(h))
        bad.append((leaves, toks, root))
    assert np.array_equal(engine.filtered_tx_verify(bad), np.where(want == 0, 1, 6))


def test_ticketed_two_outstanding(engine, cases):
    txs = [(c["leaves"], c["include"]) for c in cases]
    want = engine.filtered_tx_build(txs)
    ok = [t for t, c in enumerate(cases) if c["status"] == 0 and any(c["include"])]
    ftxs = [([x for x, f in zip(cases[t]["leaves"], cases[t]["include"]) if f], want[2][t], bytes(want[0][t]))
            for t in ok]
    t1 = engine.filtered_tx_build(txs, async_=True)
    t2 = engine.filtered_tx_build(txs[::-1], async_=True)
    t3 = engine.filtered_tx_verify(ftxs, async_=True)
    r2, r1, r3 = t2.wait(), t1.wait(), t3.wait()
    assert np.array_equal(r1[0], want[0]) and np.array_equal(r1[1], want[1]) and r1[2] == want[2]
    assert np.array_equal(r2[0], want[0][::-1]) and np.array_equal(r2[1], want[1][::-1]) and r2[2] == want[2][::-1]
    assert not r3.any()
    assert r1[2] == [c["tokens"] for c in cases]


def _device_run(engine, a):
    import torch
    dev = torch.device("cuda:0")
    g = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)  # noqa: E731
    lb, lo, tlo, inc, tko = g(a.lb), g(a.lo), g(a.tlo), g(a.inc), g(a.tko)
    txid, tok, th, cnt, st = g(a.txid), g(a.tok), g(a.th), g(a.cnt), g(a.st)
    engine.filtered_tx_build_device(lb, lo, tlo, inc, tko, txid, tok, th, cnt, st,
                                    stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    a.txid[:], a.tok[:], a.th[:], a.st[:] = txid.cpu().numpy(), tok.cpu().numpy(), th.cpu().numpy(), st.cpu().numpy()
    a.cnt[:] = cnt.cpu().numpy().view(np.uint64)


def test_device_resident_and_slot_guard(engine, cases):
    host = Arrays(cases)
    assert lib().cordahip_filtered_tx_build(engine.ctx, ctypes.byref(host.batch())) == 0
    a = Arrays(cases)
    _device_run(engine, a)
    check_against_golden(a, cases)
    for t in range(len(cases)):
        assert a.tokens(t) == host.tokens(t)
    assert np.array_equal(a.txid, host.txid) and np.array_equal(a.st, host.st) and np.array_equal(a.cnt, host.cnt)
    # one mid-batch transaction's slot one token short
    victim = next(t for t, c in enumerate(cases) if c["name"] == "random_m12")
    assert 0 < victim < len(cases) - 1 and cases[victim]["status"] == 0
    b = Arrays(cases, short={victim})
    _device_run(engine, b)
    assert b.st[victim] == _lib.TX_TOK_SLOT_TOO_SMALL and b.cnt[victim] == 0
    assert b.txid[victim].tobytes() == cases[victim]["root"]
    k0, k1 = int(b.tko[victim]), int(b.tko[victim + 1])
    assert (b.tok[k0:k1] == 0xA5).all() and (b.th[k0:k1] == 0xA5).all()  # no token written
    check_against_golden(b, cases, skip={victim})


def test_resolve_build_filtered_transactions(engine, cases):
    """resolve.build_filtered_transactions: the predicate over the components, one engine call, the
    tuples filtered_tx_verify takes; MerkleTreeException for statuses 6 and 12."""
    from corda_amd import resolve as R
    by = {c["name"]: c for c in cases}
    # the predicate sees values, not positions: cases whose selected components occur nowhere unselected
    good = [by[n] for n in ("ref_3_5", "random_m29", "random_m31", "full_33")]
    selected = {x for c in good for x, f in zip(c["leaves"], c["include"]) if f}
    assert all([x in selected for x in c["leaves"]] == [bool(f) for f in c["include"]] for c in good)
    wtxs = [R.SignedTx(components=c["leaves"], sigs=[]) if i % 2 else c["leaves"] for i, c in enumerate(good)]
    ftxs = R.build_filtered_transactions(engine, wtxs, lambda comp: comp in selected)
    for c, (leaves, toks, root) in zip(good, ftxs):
        assert leaves == [x for x, f in zip(c["leaves"], c["include"]) if f]
        assert toks == c["tokens"] and root == c["root"]
    assert not engine.filtered_tx_verify(ftxs).any()
    assert R.build_filtered_transactions(engine, [], lambda comp: True) == []
    with pytest.raises(R.MerkleTreeException, match="empty hash list"):
        R.build_filtered_transactions(engine, [good[0]["leaves"], []], lambda comp: True)
    # the count rule needs a mask that separates equal components: the engine call itself
    _, st, toks = engine.filtered_tx_build([(by["aaa_first"]["leaves"], by["aaa_first"]["include"])])
    assert st[0] == _lib.TX_HASHES_NOT_IN_TREE and toks == [[]]


def test_three_device_shards(cases, monkeypatch):
    """The shard split (offsets rebased per shard, each shard's slot range copied back to its
    place) on a context of three Device objects: CORDAHIP_TEST_DEVICE_REPLICAS, read by
    cordahip_init, as tests/test_gpu_multidevice.py uses it."""
    from corda_amd.engine import Engine
    monkeypatch.setenv("CORDAHIP_TEST_DEVICE_REPLICAS", "3")
    with Engine(1) as eng:
        assert eng.device_count() == 3
        a = Arrays(cases)
        assert lib().cordahip_filtered_tx_build(eng.ctx, ctypes.byref(a.batch())) == 0
        check_against_golden(a, cases)


@pytest.mark.parametrize("submit", [False, True])
def test_build_bad_slots(engine, cases, submit):
    a = Arrays(cases)
    before = a.outputs()

    def run(batch):
        if not submit:
            return lib().cordahip_filtered_tx_build(engine.ctx, ctypes.byref(batch))
        t = ctypes.c_uint64()
        rc = lib().cordahip_filtered_tx_build_submit(engine.ctx, ctypes.byref(batch), ctypes.byref(t))
        return rc if rc != 0 else lib().cordahip_wait(engine.ctx, t.value, -1)

    victim = next(t for t, c in enumerate(cases) if c["name"] == "random_m12")
    short = Arrays(cases, short={victim}).tko  # one slot one token short
    dec = a.tko.copy()
    dec[10] = dec[11] + 3  # decreasing
    for bad in (a.batch(tko=short), a.batch(tko=dec), a.batch(ntok=int(a.tko[a.n]) - 1)):
        assert run(bad) == INVALID
        for x, y in zip(a.outputs(), before):
            assert np.array_equal(x, y)  # outputs untouched
    assert run(a.batch()) == 0
    check_against_golden(a, cases)
