"""Required-signer coverage on the GPU (K9 tx_cover_kernel through
cordahip_tx_cover_device) and in the covered host calls, against
cordahip_cover_eval_host -- the same core on the CPU, which tests/test_cover.py
checks against the Python rule of corda_amd/resolve.py.

One 257-transaction batch (one past a 256-lane block) serves most tests: 1 to 3
Ed25519 signatures each, one transaction with 64 signatures under a 64-leaf
composite key, every case class of test_cover.py (plain keys, OR / AND / weighted
/ 2-of-3 / nested trees, shared table entries, allowed-to-be-missing, each
MALFORMED class, a transaction without required keys), corrupted signatures,
one without components and one without signatures.
"""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import test_cover as TC
from corda_amd import _lib
from corda_amd import cover as C
from corda_amd import resolve as R

pytestmark = pytest.mark.gpu
ED, K1, R1 = 4, 2, 3
NTX, BIG = 257, 200  # transaction BIG has 64 signatures and a 64-leaf composite key
CK = R.CompositeKey


def _sign(oracle, seed, msg):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_sign(seed, msg, len(msg), pub, sig)
    return pub.raw, sig.raw


def _pub(oracle, seed):
    pub = ctypes.create_string_buffer(32)
    oracle.oracle_ed25519_keypair(seed, pub)
    return pub.raw


def _oracle_id(oracle, leaves):
    out = ctypes.create_string_buffer(32)
    blob = np.frombuffer(b"".join(leaves) or b"\0", np.uint8).copy()
    off = np.zeros(len(leaves) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in leaves])
    return out.raw if oracle.oracle_tx_id(blob.ctypes.data, off.ctypes.data, len(leaves), out) == 0 else bytes(32)


def _seed(i):
    return hashlib.sha256(b"cover-signer%d" % i).digest()


# raw token streams no CompositeKey object flattens to (tokens over table keys 0 and 1)
L0, L1 = (0, 1, 0, 0), (0, 1, 0, 1)
RAW_MALFORMED = [[], [L0, L1], [L0, L1, (3, 1, 1, 0)], [(2, 1, 1, 0)], [L0, (0, 1, 0, 2**32 - 1), (2, 1, 1, 0)],
                 [L0, (1, 1, 1, 0)], [L0, L1, (2**32 - 1, 1, 1, 0)]]


@pytest.fixture(scope="module")
def batch(oracle):
    """The 257-transaction batch: leaves, signatures, the cover lists, and which
    transactions the signature half must fail."""
    rng = random.Random(257)
    txs = [[bytes(rng.getrandbits(8) for _ in range(n)) for n in (90, 40, 33)] for _ in range(NTX)]
    txs[5] = []  # no components: NO_LEAVES
    ids = [_oracle_id(oracle, tx) for tx in txs]
    pubs = [_pub(oracle, _seed(i)) for i in range(70)]
    key = [(ED, p) for p in pubs]  # (scheme, bytes) leaves
    a, b, c, d = key[0], key[1], key[2], key[3]
    n1, n2 = TC.node(a, b, threshold=1), TC.node(a, b, threshold=2)
    trees = [
        lambda s: [s[0]],                                           # the signer itself (the c4 shape)
        lambda s: [s[0], key[69]],                                  # a key nobody signs with: missing
        lambda s: [TC.node(s[0], key[69], threshold=1)],            # OR
        lambda s: [TC.node(s[0], key[69])],                         # AND, one absent
        lambda s: [],                                               # no required keys
        lambda s: [key[69], CK(0, ((s[0], 1), (key[68], 1)))],      # missing, then threshold 0: BAD_COVER wins
        lambda s: [TC.node(TC.w(n1, 13), TC.w(n2, 27))],            # CompositeKeyTests.kt:125-131
        lambda s: [TC.node(a, b, c, threshold=2)],                  # 2-of-3
        lambda s: [TC.nested_keys()[5]],                            # key6 of :215-221
        lambda s: [s[0], key[67]],                                  # key[67] is allowed to be missing
        lambda s: [s[0], TC.node(s[0], TC.node(s[0], d, threshold=1), threshold=2), s[0]],  # one entry, many leaves
        lambda s: [CK(5, ((a, 2), (b, 2)))],                        # threshold above the total
        lambda s: [CK(1, ((a, 0), (b, 1)))],                        # weight 0
        lambda s: [CK(2, ((a, 3),))],                               # one child
        lambda s: [CK(1, ((a, 2**31 - 1), (b, 2**31 - 1)))],        # Math.addExact overflow
        lambda s: [CK(2**31 - 1, ((a, 2**31 - 2), (b, 1)))],        # total exactly 2^31 - 1: valid
        lambda s: [TC.node(TC.node(a, b), c, threshold=1), d],      # (A and B) or C, and D
    ]
    sigs, must, bad_sig = [], [], set()
    for t in range(NTX):
        signers = list(range(64)) if t == BIG else [(t + j) % 4 for j in range(1 + t % 3)]
        per = []
        for i in signers:
            pub, sg = _sign(oracle, _seed(i), ids[t])
            per.append((ED, pub, sg))
        if t % 10 == 3:  # a corrupted signature (the last one)
            sg = bytearray(per[-1][2])
            sg[7] ^= 0x10
            per[-1] = (ED, per[-1][1], bytes(sg))
            bad_sig.add(t)
        sigs.append(per)
        must.append([TC.node(*key[:64])] if t == BIG else trees[t % len(trees)]([(ED, p) for _, p, _ in per]))
    sigs[11] = []  # NO_SIGNATURES
    must[BIG + 1] = [TC.node(*key[:64], threshold=63), TC.node(*key[:64], threshold=1)]  # 64 leaves, 1 to 3 signatures
    tx_reqs, keys = C.flatten_lists(must, None, allowed_to_be_missing=[key[67]])
    assert keys[0] == a and keys[1] == b  # the raw streams below name table entries 0 and 1
    for i, toks in enumerate(RAW_MALFORMED):
        t = 20 + 7 * i
        tx_reqs[t] = list(tx_reqs[t]) + [(toks, False)] + [([L0], False)]
    return {"txs": txs, "ids": ids, "sigs": sigs, "tx_reqs": tx_reqs, "keys": keys, "bad_sig": bad_sig}


def _cover(batch):
    return C.CoverArrays(batch["tx_reqs"], batch["keys"])


def _device_inputs(torch, batch):
    dev = torch.device("cuda:0")
    leaves = [x for tx in batch["txs"] for x in tx]
    flat = [x for per in batch["sigs"] for x in per]
    return dict(
        lb=torch.tensor(np.frombuffer(b"".join(leaves), np.uint8), device=dev),
        lo=torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in leaves])]).astype(np.int64), device=dev),
        tlo=torch.tensor(np.concatenate([[0], np.cumsum([len(tx) for tx in batch["txs"]])]).astype(np.int64), device=dev),
        tso=torch.tensor(np.concatenate([[0], np.cumsum([len(p) for p in batch["sigs"]])]).astype(np.int64), device=dev),
        k=torch.tensor(np.frombuffer(b"".join(x[1] for x in flat), np.uint8).reshape(-1, 32), device=dev),
        s=torch.tensor(np.frombuffer(b"".join(x[2] for x in flat), np.uint8).reshape(-1, 64), device=dev),
        txid=torch.empty((NTX, 32), dtype=torch.uint8, device=dev),
        tst=torch.empty(NTX, dtype=torch.uint8, device=dev),
        fb=torch.empty(NTX, dtype=torch.int64, device=dev),
        sst=torch.empty(len(flat), dtype=torch.uint8, device=dev))


def test_cover_kernel_after_the_signed_tx_call_on_one_stream(engine, batch):
    torch = pytest.importorskip("torch")
    x = _device_inputs(torch, batch)
    cov = _cover(batch)
    cs, ct = cov.to_device()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        engine.signed_tx_verify_ed25519_device(x["lb"], x["lo"], x["tlo"], x["tso"], x["k"], x["s"], x["txid"],
                                               x["tst"], x["fb"], x["sst"], stream=stream)
        before = x["tst"].clone()  # on the same stream: the statuses the signature half left
        engine.tx_cover_device(NTX, x["tst"], x["tso"], x["k"], cs, stream=stream)
    stream.synchronize()
    assert engine.last_kernel_ms() > 0
    before, after = before.cpu().numpy(), x["tst"].cpu().numpy()
    req, first = cov.from_device(ct)
    # the signature half: every corrupted-signature, no-leaves and no-signatures transaction failed ...
    failed = {t for t in range(NTX) if before[t] != 0}
    assert failed == batch["bad_sig"] | {5, 11}
    assert before[5] == _lib.TX_NO_LEAVES and before[11] == _lib.TX_NO_SIGNATURES
    assert all(before[t] == 1 for t in batch["bad_sig"])
    assert np.array_equal(x["txid"].cpu().numpy()[6], np.frombuffer(batch["ids"][6], np.uint8))
    # ... and keeps its earlier status through the coverage kernel
    assert all(after[t] == before[t] for t in failed)
    want_st, want_req, want_first = C.cover_eval_host(_cover(batch), before, batch["sigs"])
    assert np.array_equal(req, want_req)
    assert np.array_equal(after, want_st)
    assert np.array_equal(first, want_first)
    # the batch holds every req_status value and every outcome, the 64-leaf key among them
    assert set(req.tolist()) == {0, 1, 2, 3, 4}
    assert {0, _lib.TX_SIGNATURES_MISSING, _lib.TX_BAD_COVER} <= set(after.tolist())
    off = cov.tx_req_off
    assert after[BIG] == 0 and req[int(off[BIG])] == 0
    assert after[BIG + 1] == _lib.TX_SIGNATURES_MISSING and list(req[int(off[BIG + 1]):int(off[BIG + 2])]) == [1, 0]
    for i in range(len(RAW_MALFORMED)):
        t = 20 + 7 * i
        if before[t] == 0:
            assert after[t] == _lib.TX_BAD_COVER and req[int(off[t + 1]) - 2] == 4 and req[int(off[t + 1]) - 1] in (0, 1)


@pytest.mark.parametrize("ntx", [0, 1])
def test_cover_device_tiny_batches(engine, batch, ntx):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    sub = {"tx_reqs": batch["tx_reqs"][1:1 + ntx], "keys": batch["keys"]}
    sigs = batch["sigs"][1:1 + ntx]
    cov = _cover(sub)
    cs, ct = cov.to_device()
    so, sch, kb, ko = C.sig_key_arrays(sigs)
    tst = torch.full((max(ntx, 1),), 0, dtype=torch.uint8, device=dev)
    tso = torch.tensor(so.astype(np.int64), device=dev)
    k = torch.tensor(np.concatenate([kb, np.zeros(32, np.uint8)]), device=dev)
    engine.tx_cover_device(ntx, tst, tso, k, cs)
    torch.cuda.synchronize()
    req, first = cov.from_device(ct)
    want_st, want_req, want_first = C.cover_eval_host(_cover(sub), np.zeros(ntx, np.uint8), sigs)
    assert np.array_equal(req, want_req) and np.array_equal(first, want_first)
    assert np.array_equal(tst.cpu().numpy()[:ntx], want_st)
    if ntx:
        assert want_st[0] == _lib.TX_SIGNATURES_MISSING  # transaction 1 lacks key[69]


def test_cover_device_explicit_schemes_and_csr_keys(engine, batch):
    """d_sig_scheme / d_sig_key_off given explicitly against the dense NULL form, and
    mixed schemes: the same 32 or 33 bytes under another scheme are another key."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    statuses = np.zeros(NTX, np.uint8)
    statuses[[3, 5, 40]] = [1, _lib.TX_NO_LEAVES, 4]

    def device(sigs, cov, scheme, csr):
        cs, ct = cov.to_device()
        so, sch, kb, ko = C.sig_key_arrays(sigs)
        tst = torch.tensor(statuses[:len(sigs)], device=dev)
        tso = torch.tensor(so.astype(np.int64), device=dev)
        k = torch.tensor(np.concatenate([kb, np.zeros(32, np.uint8)]), device=dev)
        engine.tx_cover_device(len(sigs), tst, tso, k, cs,
                               sig_scheme=torch.tensor(sch, device=dev) if scheme else None,
                               sig_key_off=torch.tensor(ko.astype(np.int64), device=dev) if csr else None)
        torch.cuda.synchronize()
        return (tst.cpu().numpy(),) + cov.from_device(ct)

    def same(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x, y))

    sigs = batch["sigs"]
    want = C.cover_eval_host(_cover(batch), statuses, sigs)
    forms = [device(sigs, _cover(batch), scheme, csr) for scheme in (False, True) for csr in (False, True)]
    assert all(same(f, want) for f in forms)
    # mixed schemes over the same bytes, 32-byte rows: dense rows with the scheme array, and CSR
    rng = random.Random(5)
    keys32 = [bytes([i]) * 32 for i in range(1, 6)]
    pool = [(s, k) for k in keys32 for s in (ED, K1, R1)]
    must, msigs = [], []
    for t in range(96):
        msigs.append([rng.choice(pool) + (b"",) for _ in range(rng.randint(1, 4))])
        must.append([rng.choice(pool) if rng.random() < 0.5 else
                     TC.node(*rng.sample(pool, 3), threshold=rng.randint(1, 3)) for _ in range(rng.randint(0, 3))])
    want = C.cover_eval_host(C.flatten(must), statuses[:96], msigs)
    assert {0, 1} <= set(want[1].tolist())
    assert same(device(msigs, C.flatten(must), True, False), want)
    assert same(device(msigs, C.flatten(must), True, True), want)
    # and keys of several lengths (CSR only): 33 and 65 bytes under secp256k1 / secp256r1, 32 under Ed25519
    pool = [(K1, b"\2" * 33), (R1, b"\2" * 33), (K1, b"\4" * 65), (R1, b"\4" * 65), (ED, b"\2" * 32), (ED, b"")]
    must, msigs = [], []
    for t in range(96):
        msigs.append([rng.choice(pool) + (b"",) for _ in range(rng.randint(1, 3))])
        must.append([rng.choice(pool) if rng.random() < 0.5 else
                     TC.node(*rng.sample(pool, 3), threshold=rng.randint(1, 3)) for _ in range(rng.randint(0, 3))])
    want = C.cover_eval_host(C.flatten(must), statuses[:96], msigs)
    assert {0, 1} <= set(want[1].tolist())
    assert same(device(msigs, C.flatten(must), True, True), want)


# ---- the covered host calls -----------------------------------------------------------
def _raw_components(batch):
    return [[("raw", leaf, 0) for leaf in tx] for tx in batch["txs"]]


def _want_host(engine, batch):
    ids, st, fb, sst = engine.signed_tx_verify(batch["txs"], batch["sigs"])
    assert {t for t in range(NTX) if st[t] != 0} == batch["bad_sig"] | {5, 11}
    return (ids.copy(), fb.copy(), sst.copy()) + C.cover_eval_host(_cover(batch), st, batch["sigs"])


def _same_as(want, got):
    ids, st, fb, sst, req, first = got
    w_ids, w_fb, w_sst, w_st, w_req, w_first = want
    ok = (w_st != _lib.TX_NO_LEAVES) & (w_st != _lib.TX_NO_SIGNATURES)
    assert np.array_equal(ids[ok], w_ids[ok]) and np.array_equal(fb, w_fb) and np.array_equal(sst, w_sst)
    assert np.array_equal(st, w_st) and np.array_equal(req, w_req) and np.array_equal(first, w_first)


@pytest.mark.parametrize("chunk", ["default", "7"])
def test_four_covered_host_calls_agree(engine, batch, chunk, monkeypatch):
    """chunk 7: signature pipeline chunks of 7 lanes (CORDAHIP_TX_SIG_CHUNK), so most transactions are
    reduced -- and covered -- chunk by chunk while later chunks verify, the rest in the sweep after the drain."""
    if chunk != "default":
        monkeypatch.setenv("CORDAHIP_TX_SIG_CHUNK", chunk)
    want = _want_host(engine, batch)
    assert {0, _lib.TX_SIGNATURES_MISSING, _lib.TX_BAD_COVER, 1, 6, 7} <= set(want[3].tolist())
    _same_as(want, engine.signed_tx_verify_covered(batch["txs"], batch["sigs"], _cover(batch)))
    _same_as(want, engine.signed_txcomp_verify_covered(_raw_components(batch), batch["sigs"], _cover(batch)))
    # the ticketed forms, two in flight at once
    t1 = engine.signed_tx_verify_covered(batch["txs"], batch["sigs"], _cover(batch), async_=True)
    t2 = engine.signed_txcomp_verify_covered(_raw_components(batch), batch["sigs"], _cover(batch), async_=True)
    _same_as(want, t2.wait())
    _same_as(want, t1.wait())


@pytest.mark.parametrize("field,idx,val", [("tx_req_off", -1, 10**6), ("tx_req_off", 3, 2**63),
                                           ("req_tok_off", 10, 2**64 - 1), ("req_tok_off", 1, 10**7),
                                           ("ckey_off", 2, 31), ("ckey_off", -1, 10**6)])
def test_bad_cover_offsets_fail_the_call_only(engine, batch, field, idx, val):
    want = _want_host(engine, batch)
    for comps in (False, True):
        cov = _cover(batch)
        getattr(cov, field)[idx] = val
        with pytest.raises(_lib.EngineError) as e:
            if comps:
                engine.signed_txcomp_verify_covered(_raw_components(batch), batch["sigs"], cov)
            else:
                engine.signed_tx_verify_covered(batch["txs"], batch["sigs"], cov)
        assert e.value.code == -1
        with pytest.raises(_lib.EngineError) as e:  # the ticketed form reports it at wait
            engine.signed_tx_verify_covered(batch["txs"], batch["sigs"], cov, async_=True).wait()
        assert e.value.code == -1
    _same_as(want, engine.signed_tx_verify_covered(batch["txs"], batch["sigs"], _cover(batch)))  # still usable


def test_stack_scratch_is_accounted_and_trimmed(engine, batch):
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    cov = _cover(batch)
    cs, ct = cov.to_device()
    so, sch, kb, ko = C.sig_key_arrays(batch["sigs"])
    tst = torch.zeros(NTX, dtype=torch.uint8, device=dev)
    tso = torch.tensor(so.astype(np.int64), device=dev)
    k = torch.tensor(kb, device=dev)
    engine.trim()
    base = engine.device_mem()[0]
    engine.tx_cover_device(NTX, tst, tso, k, cs)
    torch.cuda.synchronize()
    assert engine.device_mem()[0] - base == 8 * cov.ntok  # one 8-byte slot per token
    engine.tx_cover_device(NTX, tst, tso, k, cs)  # grow-only: a second call reuses it
    torch.cuda.synchronize()
    assert engine.device_mem()[0] - base == 8 * cov.ntok
    engine.trim()
    assert engine.device_mem()[0] == base
