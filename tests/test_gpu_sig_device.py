"""The generic mixed-scheme batch resident in HBM (K23: cordahip_sig_verify_device): classified,
packed and verified on the GPU. Every lane's status is compared with the CPU oracle (Ed25519,
ECDSA, unsupported schemes), the Python model of RSASSA-PSS (tests/golden/bc_rsa_pss.py) and the
host call cordahip_sig_verify on the same rows.

The device call takes dense message rows of one length, so the adversarial mix of
test_gpu_host_batch.make_batch (message lengths 0, 1, 31, 32, 33, 64, 100, 137) goes through it
as one call per message length: that covers msg_len 0 (EMPTY under doVerify, hashed under
isValid) and both row gathers (aligned 32-byte rows, any other length)."""
import random

import numpy as np
import pytest

import bc_rsa_pss as bc
from corda_amd import _lib
from test_gpu_host_batch import make_batch, oracle_status
from test_gpu_rsa_route import by_class, load_keys, pooled

pytestmark = pytest.mark.gpu
RSA, ED = 1, 4
BAD_RANGE = 19


def rsa_rows(n=200):
    """(RSA, key, sig, msg) lanes over the golden keys of all three width classes: valid, a flipped
    bit, an empty and an over-long signature, a truncated key (BAD_KEY), an even modulus (UNSUPPORTED)"""
    keys = load_keys()
    per = [by_class(keys, w) for w in (64, 96, 128)]
    rows = []
    for i in range(n):
        k = per[i % 3][(i // 3) % len(per[i % 3])]
        m, sig = pooled(k, i, flip=i % 4 == 3)
        der = k["der"]
        if i % 11 == 5:
            sig = b""
        elif i % 11 == 6:
            sig = sig + b"\0"
        elif i % 11 == 7:
            der = der[:-1]
        elif i % 11 == 8:
            der = bc.encode_key(k["n"] + 1, k["e"])
        rows.append((RSA, der, sig, m))
    return rows


def model_status(oracle, rows, is_valid, rsa=True):
    want = oracle_status(oracle, rows, is_valid)
    if rsa:
        for i, (sch, k, s, m) in enumerate(rows):
            if sch == RSA:
                want[i] = bc.verify(k, s, m, is_valid=is_valid)
    return want


@pytest.fixture(scope="module")
def mix(oracle):
    """the adversarial mix, shuffled, and its lanes grouped by message length"""
    rows = make_batch(oracle, n=2600) + rsa_rows(200)
    random.Random(23).shuffle(rows)
    groups = {}
    for i, r in enumerate(rows):
        groups.setdefault(len(r[3]), []).append(i)
    return rows, groups


def csr(parts):
    off = np.zeros(len(parts) + 1, np.int64)
    if parts:
        off[1:] = np.cumsum([len(p) for p in parts])
    return np.frombuffer(b"".join(parts), np.uint8).copy(), off


class Dev:
    """a batch's tensors on the GPU"""

    def __init__(self, rows, msg_len, msg_row=None, msgs=None, tail=0):
        import torch
        self.torch, self.n = torch, len(rows)
        dev = torch.device("cuda:0")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        kb, ko = csr([r[1] for r in rows])
        sb, so = csr([r[2] for r in rows])
        self.key_bytes, self.sig_bytes = kb.size, sb.size
        # `tail` canary bytes behind the declared buffers
        self.key = t(np.concatenate([kb, np.full(tail, 0xA5, np.uint8)]))
        self.sig = t(np.concatenate([sb, np.full(tail, 0xA5, np.uint8)]))
        self.ko, self.so = ko, so
        self.scheme = t(np.array([r[0] for r in rows], np.uint8))
        if msgs is None:
            msgs = [r[3] for r in rows]
        m = np.frombuffer(b"".join(msgs), np.uint8).reshape(len(msgs), msg_len) if msg_len else \
            np.zeros((len(msgs), 0), np.uint8)
        self.msgs = t(m.copy())
        self.msg_row = None if msg_row is None else t(np.asarray(msg_row, np.int32))
        self.status = torch.full((self.n + 64,), 0xEE, dtype=torch.uint8, device=dev)
        self.verdict = torch.zeros(((self.n + 63) // 64 + 1,), dtype=torch.int64, device=dev)

    def run(self, engine, is_valid=False, rsa=True, verdict=True, stream=None):
        t = self.torch
        dev = self.key.device
        engine.sig_verify_device(self.scheme, self.key, t.from_numpy(self.ko).to(dev), self.sig,
                                 t.from_numpy(self.so).to(dev), self.msgs, self.status[:self.n],
                                 self.verdict if verdict else None, msg_row=self.msg_row, is_valid=is_valid,
                                 rsa_on_device=rsa, stream=stream, key_bytes=self.key_bytes, sig_bytes=self.sig_bytes)

    def result(self):
        st = self.status.cpu().numpy()
        assert (st[self.n:] == 0xEE).all()  # nothing written past the batch
        return [int(x) for x in st[:self.n]]

    def verdict_bits(self):
        v = self.verdict.cpu().numpy().view(np.uint64)
        assert int(v[-1]) == 0
        return [(int(v[i // 64]) >> (i % 64)) & 1 for i in range(self.n)]


def run_rows(engine, rows, msg_len, **kw):
    d = Dev(rows, msg_len)
    d.run(engine, **kw)
    d.torch.cuda.synchronize()
    return d.result(), d.verdict_bits()


def mismatches(rows, got, want):
    return [(i, rows[i][0], len(rows[i][1]), len(rows[i][2]), len(rows[i][3]), g, w)
            for i, (g, w) in enumerate(zip(got, want)) if g != w][:12]


# ---- 1. the adversarial mix against the oracle, the model and the host call -----------------------
@pytest.mark.parametrize("is_valid", [False, True])
def test_mix_vs_oracle_and_host_call(engine, oracle, mix, is_valid):
    rows, groups = mix
    want = model_status(oracle, rows, is_valid)
    host, _ = engine.verify_batch(*zip(*rows), is_valid=is_valid, rsa=True)
    assert [int(x) for x in host] == want
    assert len(groups) == 8 and 0 in groups and 32 in groups
    seen = set()
    for ln, idx in sorted(groups.items()):
        sub = [rows[i] for i in idx]
        got, bits = run_rows(engine, sub, ln, is_valid=is_valid, rsa=True)
        assert not mismatches(sub, got, [want[i] for i in idx]), (ln, mismatches(sub, got, [want[i] for i in idx]))
        assert bits == [int(g == 0) for g in got]
        seen |= {(sub[j][0], got[j]) for j in range(len(sub))}
    # the three families were accepted and rejected, RSA keys were declined both ways
    for sch in (RSA, 2, 3, ED):
        assert (sch, _lib.OK) in seen and (sch, _lib.BAD_SIG) in seen, (sch, sorted(seen))
    assert (RSA, _lib.BAD_KEY) in seen and (RSA, _lib.UNSUPPORTED) in seen


def test_without_the_rsa_flag_rsa_lanes_are_unsupported(engine, oracle, mix):
    rows, groups = mix
    sub = [rows[i] for i in groups[32]]
    got, bits = run_rows(engine, sub, 32, rsa=False)
    want = model_status(oracle, sub, False, rsa=False)
    # the 200 RSA rows and make_batch's few scheme-1 lanes
    assert sum(r[0] == RSA for r in sub) >= 200 and all(w == _lib.UNSUPPORTED for r, w in zip(sub, want) if r[0] == RSA)
    assert not mismatches(sub, got, want), mismatches(sub, got, want)
    assert bits == [int(g == 0) for g in got]


# ---- 2. edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_small_batches(engine, oracle, mix, n):
    rows, groups = mix
    sub = [rows[i] for i in groups[32][:n]]
    got, bits = run_rows(engine, sub, 32)
    assert got == model_status(oracle, sub, False) and bits == [int(g == 0) for g in got]


def test_one_class_owns_every_lane(engine, oracle, mix):
    rows, groups = mix
    sub = [rows[i] for i in groups[32]]
    keys = load_keys()
    picks = {
        "ed25519": [r for r in sub if r[0] == ED and len(r[1]) == 32],
        "ecdsa": [r for r in sub if r[0] in (2, 3) and len(r[1]) in (33, 65)],
        "direct": [r for r in sub if r[0] not in (RSA, 2, 3, ED)],
    }
    for w in (64, 96, 128):
        # the lanes of the class whose verdict needs the arithmetic: a whole key, a signature of the modulus' length
        sig_bytes = {k["der"]: (k["n"].bit_length() + 7) // 8 for k in by_class(keys, w)}
        picks["rsa%d" % w] = [r for r in sub if r[0] == RSA and sig_bytes.get(r[1]) == len(r[2])]
    for name, lanes in picks.items():
        lanes = lanes[:130]
        assert len(lanes) >= 10, name
        got, bits = run_rows(engine, lanes, 32)
        assert got == model_status(oracle, lanes, False), name
        assert bits == [int(g == 0) for g in got], name
    # every lane's message row out of bounds: the bad-range class alone
    lanes = picks["ed25519"][:70]
    d = Dev(lanes, 32, msg_row=[len(lanes) + j for j in range(len(lanes))])
    d.run(engine)
    d.torch.cuda.synchronize()
    assert d.result() == [BAD_RANGE] * len(lanes) and d.verdict_bits() == [0] * len(lanes)


def test_verdict_null_and_msg_row_forms(engine, oracle, mix):
    rows, groups = mix
    sub = [rows[i] for i in groups[32][:300]]
    want = model_status(oracle, sub, False)
    d = Dev(sub, 32)
    d.run(engine, verdict=False)
    d.torch.cuda.synchronize()
    assert d.result() == want and not d.verdict.cpu().numpy().any()
    ident = Dev(sub, 32, msg_row=list(range(len(sub))))
    ident.run(engine)
    ident.torch.cuda.synchronize()
    assert ident.result() == want
    # many lanes, few rows (the signed-tx shape): each lane signs one of 7 messages; a lane
    # pointed at another row than the one it signed must fail exactly as the oracle says
    rng = random.Random(7)
    msgs = [sub[j][3] for j in range(7)]
    lanes, row_of = [], []
    for j in range(400):
        src = sub[rng.randrange(len(sub))]
        if src[3] in msgs and rng.random() < 0.8:
            r = msgs.index(src[3])
        else:
            r = rng.randrange(7)
        lanes.append((src[0], src[1], src[2], msgs[r]))
        row_of.append(r)
    for j in range(7):  # every row is signed by its own lane at least once
        lanes.append(sub[j])
        row_of.append(j)
    few = Dev(lanes, 32, msg_row=row_of, msgs=msgs)
    few.run(engine)
    few.torch.cuda.synchronize()
    want_few = model_status(oracle, lanes, False)
    assert few.result() == want_few and want_few.count(0) >= 5 and want_few.count(1) >= 100


# ---- 3. bad ranges ---------------------------------------------------------------------------------
def test_bad_ranges_are_per_lane_and_never_read(engine, oracle, mix):
    rows, groups = mix
    sub = [rows[i] for i in groups[32][:200]]
    n = len(sub)
    tail = 4096  # the allocations really extend this far: every offset used stays inside them
    d = Dev(sub, 32, msg_row=list(range(n)), tail=tail)
    a, c = 77, 140
    d.ko = d.ko.copy()
    d.so = d.so.copy()
    d.ko[a] = d.ko[a + 1] + 5            # lane a: reversed key range (lane a - 1 gets a longer key)
    d.so[n] = d.sig_bytes + 100          # the last lane: its signature reaches past sig_bytes
    mr = list(range(n))
    mr[c] = n                            # lane c: msg_row >= msg_rows
    d.msg_row = d.torch.from_numpy(np.asarray(mr, np.int32)).to(d.key.device)
    d.run(engine)
    d.torch.cuda.synchronize()
    got = d.result()
    kb, sb = d.key.cpu().numpy(), d.sig.cpu().numpy()
    assert (kb[d.key_bytes:] == 0xA5).all() and (sb[d.sig_bytes:] == 0xA5).all() and kb.size == d.key_bytes + tail
    # every other lane: the oracle's status of the bytes its offsets name
    eff = [(sub[i][0], bytes(kb[d.ko[i]:d.ko[i + 1]]), bytes(sb[d.so[i]:d.so[i + 1]]), sub[i][3]) for i in range(n)]
    want = model_status(oracle, [e if i not in (a, c, n - 1) else sub[i] for i, e in enumerate(eff)], False)
    for i in (a, c, n - 1):
        want[i] = BAD_RANGE
    assert got == want, mismatches(eff, got, want)
    assert d.verdict_bits() == [int(g == 0) for g in got]


# ---- 6. two enqueues back to back on one stream ----------------------------------------------------
def test_two_enqueues_on_one_stream_without_a_sync(engine, oracle, mix):
    import torch
    rows, groups = mix
    big = [rows[i] for i in groups[32]]
    small = [rows[i] for i in groups[64][:97]]
    ed_only = [r for r in big if r[0] == ED][:333]
    s = torch.cuda.Stream()
    devs = [Dev(big, 32), Dev(small, 64), Dev(ed_only, 32)]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        devs[0].run(engine, stream=s)
        devs[1].run(engine, is_valid=True, rsa=False, stream=s)
        devs[2].run(engine, stream=s)
    s.synchronize()
    assert devs[0].result() == model_status(oracle, big, False)
    assert devs[1].result() == model_status(oracle, small, True, rsa=False)
    assert devs[2].result() == model_status(oracle, ed_only, False)
    for d in devs:
        assert d.verdict_bits() == [int(g == 0) for g in d.result()]


# ---- 4. signed transactions: the mixed device calls against the host calls -------------------------
def _signers():
    """id -> (scheme, key, sig) makers of the three families (ECDSA and RSA sign in Python: use sparingly)"""
    import ctypes
    import hashlib

    import bc_ecdsa as ec
    from test_gpu_rsa_route import sign as rsa_sign
    keys = load_keys()
    rsa_keys = [by_class(keys, w)[0] for w in (64, 96, 128)]
    rng = random.Random(41)

    def ed(oracle, j, msg):
        pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
        oracle.oracle_ed25519_sign(hashlib.sha256(b"sd%d" % (j % 20)).digest(), msg, len(msg), pub, sig)
        return (ED, pub.raw, sig.raw)

    def ecdsa(j, msg):
        sch = 2 + j % 2
        d = 1 + (j * 7919) % 1000003
        pk = ec.keypair(sch, d)
        rr, ss = ec.sign(sch, d, msg, rng.randrange(1, ec.CURVES[sch].n))
        return (sch, ec.compress(pk) if j % 3 == 0 else pk, ec.der_encode(rr, ss))

    def rsa(j, msg):
        k = rsa_keys[j % 3]
        return (RSA, k["der"], rsa_sign(rng, k, msg))

    return ed, ecdsa, rsa


def _mixed_sigs(oracle, ids, pool, every=5):
    """1-3 signatures per transaction: Ed25519 over the id, every few transactions an ECDSA and an
    RSA signer, now and then a lane drawn from the adversarial pool (signed over something else,
    malformed, unsupported) and a flipped bit"""
    ed, ecdsa, rsa = _signers()
    rng = random.Random(43)
    sigs = []
    for t, txid in enumerate(ids):
        msg = txid if txid else bytes(32)
        per = [ed(oracle, t, msg)]
        if t % every == 1:
            per.append(ecdsa(t, msg))
        if t % every == 3:
            per.append(rsa(t, msg))
        if t % 4 == 2:
            per.append(ed(oracle, t + 1, msg))
        if t % 9 == 4:
            p = pool[rng.randrange(len(pool))]
            per.insert(rng.randrange(len(per) + 1), (p[0], p[1], p[2]))
        if t % 13 == 6:
            q = rng.randrange(len(per))
            g = bytearray(per[q][2])
            g[len(g) // 2] ^= 2
            per[q] = (per[q][0], per[q][1], bytes(g))
        sigs.append(per[:3])
    return sigs


def _dev_sig_args(torch, dev, sigs):
    flat = [x for per in sigs for x in per]
    so = np.zeros(len(sigs) + 1, np.int64)
    so[1:] = np.cumsum([len(per) for per in sigs])
    kb, ko = csr([x[1] for x in flat])
    sb, sgo = csr([x[2] for x in flat])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    n = len(sigs)
    outs = (torch.zeros((max(n, 1), 32), dtype=torch.uint8, device=dev), torch.zeros(max(n, 1), dtype=torch.uint8, device=dev),
            torch.zeros(max(n, 1), dtype=torch.int64, device=dev),
            torch.full((max(len(flat), 1),), 0xEE, dtype=torch.uint8, device=dev))
    return t(so), (t(np.array([x[0] for x in flat], np.uint8)), t(kb), t(ko), t(sb), t(sgo)), outs, len(flat)


def _results(outs, n, nsig):
    return tuple(o.cpu().numpy()[:k] for o, k in zip(outs, (n, n, n, nsig)))


def _same_results(a, b, ctx):
    """(ids, tx_status, first_bad, sig_status) of two calls; a transaction without an id has none to compare"""
    for x, y, name in zip(a[1:], b[1:], ("tx_status", "first_bad", "sig_status")):
        assert np.array_equal(np.asarray(x), np.asarray(y)), (ctx, name, np.nonzero(np.asarray(x) != np.asarray(y))[0][:8])
    has_id = ~np.isin(np.asarray(b[1]), (_lib.TX_NO_LEAVES, _lib.TX_BAD_COMPONENT))
    assert np.array_equal(np.asarray(a[0])[has_id], np.asarray(b[0])[has_id]), (ctx, "ids")


def test_signed_tx_device_equals_host_call(engine, oracle, mix):
    import torch
    dev = torch.device("cuda:0")
    rows, groups = mix
    pool = [rows[i] for i in groups[32]]
    rng = random.Random(47)
    ntx = 300
    txs = [[bytes(rng.getrandbits(8) for _ in range(rng.choice((33, 150, 450)))) for _ in range(rng.choice((1, 2, 3, 4)))]
           for _ in range(ntx)]
    txs[9] = []  # no leaves
    ids, _ = engine.tx_ids(txs)
    sigs = _mixed_sigs(oracle, [ids[t].tobytes() for t in range(ntx)], pool)
    sigs[20] = []  # no signatures
    e0 = sigs[30][0]
    sigs[30] = [e0, (e0[0], e0[1], e0[2][:10] + bytes([e0[2][10] ^ 1]) + e0[2][11:])]  # the second signature is bad
    leaves = [x for tx in txs for x in tx]
    lb = torch.from_numpy(np.frombuffer(b"".join(leaves), np.uint8).copy()).to(dev)
    lo = torch.from_numpy(np.concatenate([[0], np.cumsum([len(x) for x in leaves])]).astype(np.int64)).to(dev)
    tlo = torch.from_numpy(np.concatenate([[0], np.cumsum([len(tx) for tx in txs])]).astype(np.int64)).to(dev)
    try:
        for on in (True, False):
            engine.set_rsa_on_device(on)
            host = engine.signed_tx_verify(txs, sigs)
            tso, sg, outs, nsig = _dev_sig_args(torch, dev, sigs)
            engine.signed_tx_verify_device(lb, lo, tlo, tso, *sg, *outs)
            torch.cuda.synchronize()
            got = _results(outs, ntx, nsig)
            _same_results(got, host, "rsa_on_device=%s" % on)
            flat = [x for per in sigs for x in per]
            rsa_st = {int(got[3][i]) for i, x in enumerate(flat) if x[0] == RSA and len(x[1]) > 100}
            assert (_lib.OK in rsa_st) if on else rsa_st == {_lib.UNSUPPORTED}, rsa_st
            assert got[1][9] == _lib.TX_NO_LEAVES and got[1][20] == _lib.TX_NO_SIGNATURES
            assert got[1][30] == _lib.BAD_SIG and got[2][30] == 1
            assert (got[1] == 0).sum() > ntx // 3
            for sch in (2, 3, ED):
                assert _lib.OK in {int(got[3][i]) for i, x in enumerate(flat) if x[0] == sch}, sch
            assert (got[3] == _lib.BAD_SIG).sum() > 10
    finally:
        engine.set_rsa_on_device(False)


def _comp_corpora(engine, oracle):
    """(name, blob, items, tx_item_off, ids) of the payment corpus and a cash-issue corpus"""
    from corda_amd.corpus import cash_issue_items
    from test_gpu_kryo_payment import _corpus
    c, _, ids, ed_sigs = _corpus(oracle, 67)
    yield "payments", c["blob"], c["items"], np.asarray(c["tx_item_off"], np.uint64), ids, ed_sigs
    g = np.random.default_rng(5)
    ntx = 120
    blob, items, _ = cash_issue_items(g.integers(0, 256, (ntx, 32), dtype=np.uint8),
                                      g.integers(0, 256, (ntx, 32), dtype=np.uint8), bytes(range(32)),
                                      g.integers(1, 10**9, ntx), g.integers(-2**63, 2**63 - 1, ntx))
    it = items.reshape(-1).copy()
    host_it = it.copy()
    host_it["data"] += np.uint64(blob.ctypes.data)
    hb, ho = _lib.kryo_encode_array(host_it)
    leaves = [[hb[int(ho[5 * t + j]):int(ho[5 * t + j + 1])].tobytes() for j in range(5)] for t in range(ntx)]
    ids_l, _ = engine.tx_ids(leaves)
    yield "cash issues", blob, it, np.arange(0, 5 * ntx + 1, 5, dtype=np.uint64), [x.tobytes() for x in ids_l], None


def _dev_comp(engine, torch, dev, blob, items, tio, sigs, mixed=True):
    n = len(tio) - 1
    d_items = torch.from_numpy(np.ascontiguousarray(items).view(np.uint8).copy()).to(dev)
    d_blob = torch.from_numpy(np.ascontiguousarray(blob, dtype=np.uint8).copy()).to(dev)
    d_tio = torch.from_numpy(np.asarray(tio, np.int64)).to(dev)
    tso, sg, outs, nsig = _dev_sig_args(torch, dev, sigs)
    if mixed:
        engine.signed_txcomp_verify_device(d_items, len(items), d_blob, d_tio, tso, *sg, *outs)
    else:
        flat = [x for per in sigs for x in per]
        k = torch.from_numpy(np.frombuffer(b"".join(x[1] for x in flat), np.uint8).reshape(-1, 32).copy()).to(dev)
        s = torch.from_numpy(np.frombuffer(b"".join(x[2] for x in flat), np.uint8).reshape(-1, 64).copy()).to(dev)
        engine.signed_txcomp_verify_ed25519_device(d_items, len(items), d_blob, d_tio, tso, k, s, *outs)
    torch.cuda.synchronize()
    return _results(outs, n, nsig)


def test_signed_txcomp_device_equals_host_call(engine, oracle, mix):
    import torch
    dev = torch.device("cuda:0")
    rows, groups = mix
    pool = [rows[i] for i in groups[32]]
    try:
        for name, blob, items, tio, ids, _ in _comp_corpora(engine, oracle):
            sigs = _mixed_sigs(oracle, ids, pool, every=7)
            flat = [x for per in sigs for x in per]
            assert {x[0] for x in flat} >= {RSA, 2, 3, ED}
            for on in (True, False):
                engine.set_rsa_on_device(on)
                host = engine.signed_txcomp_verify_arrays(blob, items, tio, sigs)
                got = _dev_comp(engine, torch, dev, blob, items, tio, sigs)
                _same_results(got, host, (name, on))
                assert [x.tobytes() for x in got[0]] == ids and (got[1] == 0).sum() > len(ids) // 3, name
                rsa_st = {int(got[3][i]) for i, x in enumerate(flat) if x[0] == RSA and len(x[1]) > 100}
                assert (_lib.OK in rsa_st) if on else rsa_st == {_lib.UNSUPPORTED}, (name, rsa_st)
    finally:
        engine.set_rsa_on_device(False)


# ---- 5. an all-Ed25519 batch: the mixed call answers what the Ed25519-only call answers ------------
def test_all_ed25519_txcomp_is_byte_identical(engine, oracle):
    import torch
    from test_gpu_kryo_payment import _corpus
    dev = torch.device("cuda:0")
    c, _, ids, sigs = _corpus(oracle, 300)
    a = _dev_comp(engine, torch, dev, c["blob"], c["items"], c["tx_item_off"], sigs, mixed=True)
    b = _dev_comp(engine, torch, dev, c["blob"], c["items"], c["tx_item_off"], sigs, mixed=False)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert (a[1] == 1).sum() >= 2 and (a[1] == 0).sum() > 150


def test_overlapping_key_ranges_do_not_overrun_the_rsa_rows(engine, oracle):
    """key_off = [0, L, 0, L, ...]: every even lane a valid RSA lane over the SAME key bytes, every odd
    lane reversed. The RSA classes' rows are sized from key_bytes, which such offsets defeat: the class
    holds key_bytes / 131 = 2 rows, the other even lanes are BAD_RANGE, nothing past the rows is
    touched and every lane has a definite status."""
    k = by_class(load_keys(), 64)[0]
    n = 600  # several tiles' worth of lanes past the class's two rows, and past a gather block
    rows = []
    for i in range(n):
        m, sig = pooled(k, i // 2, flip=i % 8 == 6)
        rows.append((RSA, k["der"] if i == 0 else b"", sig, m))
    d = Dev(rows, 32, tail=256)
    ln = len(k["der"])
    assert d.key_bytes == ln and ln // 131 == 2
    d.ko = np.array([0 if i % 2 == 0 else ln for i in range(n + 1)], np.int64)
    d.run(engine)
    d.torch.cuda.synchronize()
    got = d.result()
    want = [BAD_RANGE] * n
    for i in (0, 2):  # the class's two rows, in lane order
        want[i] = bc.verify(k["der"], rows[i][2], rows[i][3])
    assert got == want and want[0] == _lib.OK
    assert d.verdict_bits() == [int(g == 0) for g in got]
    # and the scratch is sound afterwards: an ordinary batch right behind it
    sub = rsa_rows(60)
    got2, _ = run_rows(engine, sub, 32)
    assert got2 == model_status(oracle, sub, False)


def test_invalid_arguments_are_refused_before_any_enqueue(engine):
    import ctypes

    import torch
    from corda_amd._lib import lib
    dev = torch.device("cuda:0")
    z = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device=dev)  # noqa: E731
    sch, key, sig, msgs, st = z(4), z(64), z(64), z(4 * 32), torch.full((4,), 0xEE, dtype=torch.uint8, device=dev)
    ko, so, mr, vd = z(6, torch.int64), z(6, torch.int64), z(5, torch.int32), z(2, torch.int64)
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)  # noqa: E731
    f = lib().cordahip_sig_verify_device
    ctx = engine._ctx

    def call(device=0, scheme=p(sch), key_off=p(ko), sig_off=p(so), msg_row=p(mr), n=4, flags=0, status=p(st),
             verdict=p(vd), msgs_p=p(msgs)):
        return f(ctx, device, scheme, p(key), key_off, 64, p(sig), sig_off, 64, msgs_p, 32, msg_row, 4, n, flags,
                 status, verdict, None)

    assert call(flags=4) == -1 and call(flags=0x80000000) == -1      # unknown flag bits
    assert call(key_off=p(ko, 4)) == -1 and call(sig_off=p(so, 1)) == -1  # offsets not 8-byte aligned
    assert call(msg_row=p(mr, 2)) == -1 and call(verdict=p(vd, 4)) == -1
    assert call(scheme=None) == -1 and call(key_off=None) == -1 and call(sig_off=None) == -1
    assert call(status=None) == -1 and call(msgs_p=None) == -1
    assert call(device=99) == -1 and call(n=1 << 31) == -1 and call(n=(1 << 63)) == -1
    assert f(None, 0, p(sch), p(key), p(ko), 64, p(sig), p(so), 64, p(msgs), 32, None, 4, 4, 0, p(st), None, None) == -1
    g = lib().cordahip_signed_tx_verify_device
    assert g(ctx, 0, None, p(ko), 0, p(ko), 1, p(ko), p(sch), p(key), p(ko, 4), 64, p(sig), p(so), 64, 1, p(msgs),
             p(st), p(vd), p(st), None) == -1  # misaligned key offsets
    assert g(ctx, 0, None, p(ko), 0, p(ko), 1, p(ko), None, p(key), p(ko), 64, p(sig), p(so), 64, 1, p(msgs),
             p(st), p(vd), p(st), None) == -1  # no scheme bytes
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0xEE).all()  # nothing was enqueued
    assert call(n=0) == 0 and call(msg_row=None, verdict=None) == 0  # and the context is usable
    torch.cuda.synchronize()
