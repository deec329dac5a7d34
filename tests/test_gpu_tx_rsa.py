"""RSA_SHA256 lanes in the signed-transaction host calls (cordahip_set_rsa_on_device): with the switch
off every RSA lane is UNSUPPORTED, as before; with it on, sig_status, first_bad_sig, tx_status and
txid equal a Python evaluation -- each RSA lane by tests/golden/bc_rsa_pss.py over the
transaction's id under doVerify rules, the ids by the C oracle -- under CORDAHIP_TX_SLICES unset
and 3 with 7-signature chunks, through the leaf, the covered, the component and the ticketed
forms, and with the RSA lanes routed to registered keys (cordahip_vkey_set_routing_rsa)."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import bc_rsa_pss as bc
import ecdsa_sign_model as ecm
from corda_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RSA, K1, R1, ED = 1, 2, 3, 4
NO_LEAVES, NO_SIGS = 6, 7


def load_keys():
    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        g = json.load(f)
    out = {}
    for k in g["keys"]:
        k = dict(k, der=bytes.fromhex(k["der"]))
        for name in ("n", "e", "d", "p", "q"):
            if name in k:
                k[name] = int(k[name], 16)
        out[k["name"]] = k
    return out


def rsa_sign(rng, k, msg):
    em = bc.encode_em(msg, k["n"].bit_length(), rng.randbytes(32))
    return bc.sign_crt(em, k["p"], k["q"], k["d"]).to_bytes((k["n"].bit_length() + 7) // 8, "big")


def ed_sign(oracle, seed, msg):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_sign(seed, msg, len(msg), pub, sig)
    return pub.raw, sig.raw


def oracle_id(oracle, leaves):
    out = ctypes.create_string_buffer(32)
    blob = np.frombuffer(b"".join(leaves) or b"\0", np.uint8).copy()
    off = np.zeros(len(leaves) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in leaves])
    rc = oracle.oracle_tx_id(blob.ctypes.data, off.ctypes.data, len(leaves), out)
    return out.raw if rc == 0 else None


@pytest.fixture(scope="module")
def eng():
    from corda_amd.engine import Engine
    with Engine(1) as e:
        yield e
        e.set_rsa_on_device(False)


class Batch:
    """about 40 transactions of 1 to 3 signatures over the three families, with the model's answers:
    lane[t][j] = the lane's own status by the model (before the transaction's reduce)"""

    def __init__(self, oracle, seed=0x7A):
        rng = random.Random(seed)
        ks = load_keys()
        self.rsa_keys = [ks["openssl_3072"], ks["openssl_2048"], ks["openssl_4096"], ks["py_2048_e3"]]
        self.notary = self.rsa_keys[0]
        self.txs = [[rng.randbytes(n) for n in (90, 40, 33)] for _ in range(42)]
        self.txs[20] = []  # no leaves, an RSA signature among its lanes
        self.ids = [oracle_id(oracle, tx) for tx in self.txs]
        ec_d = rng.randrange(1, ecm.CURVES[K1].n)
        ec_pub = ecm.public_key(ecm.CURVES[K1], ec_d)
        self.sigs, self.lane = [], []

        def lane(kind, t, bad=False):
            msg = self.ids[t] or bytes(32)
            if kind == ED:
                pub, sig = ed_sign(oracle, hashlib.sha256(b"txrsa%d" % t).digest(), msg)
                if bad:
                    sig = sig[:3] + bytes([sig[3] ^ 2]) + sig[4:]
                return (ED, pub, sig), bc.BAD_SIG if bad else bc.OK
            if kind == K1:
                sig = ecm.sign(ecm.CURVES[K1], ec_d, hashlib.sha256(b"other").digest() if bad else msg)
                return (K1, ec_pub, sig), bc.BAD_SIG if bad else bc.OK
            k = self.rsa_keys[0] if t % 2 == 0 else self.rsa_keys[t % len(self.rsa_keys)]
            sig = rsa_sign(rng, k, msg)
            if bad:
                sig = sig[:7] + bytes([sig[7] ^ 0x10]) + sig[8:]
            return (RSA, k["der"], sig), bc.verify(k["der"], sig, msg)

        for t in range(42):
            per, sts = [], []
            kinds = [(RSA,), (ED, RSA), (RSA, ED), (ED, RSA, K1), (K1, ED, RSA), (ED,), (RSA, RSA)][t % 7]
            for kind in kinds:
                x, st = lane(kind, t)
                per.append(x)
                sts.append(st)
            self.sigs.append(per)
            self.lane.append(sts)

        def replace(t, j, kind, bad=True):
            self.sigs[t][j], self.lane[t][j] = lane(kind, t, bad)

        replace(3, 1, RSA)            # the first bad signature is an RSA lane between two good ones
        replace(10, 0, ED)            # an RSA lane (good) after an earlier bad Ed25519 lane
        replace(17, 0, ED)
        replace(17, 1, RSA)           # both bad: the Ed25519 lane comes first
        replace(4, 2, RSA)            # a bad RSA lane last
        replace(6, 1, RSA)            # two RSA lanes, the second bad
        self.sigs[8][1] = (RSA, b"\x30\x03\x02\x01", self.sigs[8][1][2])  # a direct status: BAD_KEY DER
        self.lane[8][1] = bc.verify(self.sigs[8][1][1], self.sigs[8][1][2], self.ids[8])
        assert self.lane[8][1] == bc.BAD_KEY
        self.sigs[14][0] = (RSA, self.sigs[14][0][1], b"")  # an empty signature: EMPTY under doVerify
        self.lane[14][0] = bc.EMPTY
        self.sigs[21][0] = (RSA, self.sigs[21][0][1], self.sigs[21][0][2] + b"\0")  # longer than the modulus
        self.lane[21][0] = bc.BAD_SIG
        self.sigs[30] = []            # no signatures
        self.lane[30] = []
        assert any(x[0] == RSA for x in self.sigs[20])
        assert self.lane[3] == [bc.OK, bc.BAD_SIG, bc.OK] and self.lane[10] == [bc.BAD_SIG, bc.OK, bc.OK]

    def rsa_lanes(self):
        return [(t, j) for t, per in enumerate(self.sigs) for j, x in enumerate(per) if x[0] == RSA]

    def want(self, rsa_on):
        """(tx_status, first_bad, sig_status flat) by SignedTransaction's order of checks"""
        tx_st, first, flat = [], [], []
        for t, per in enumerate(self.sigs):
            lanes = [st if (x[0] != RSA or rsa_on) else bc.UNSUPPORTED for x, st in zip(per, self.lane[t])]
            if not per:
                tx_st.append(NO_SIGS)
                first.append(-1)
                continue
            if not self.txs[t]:
                tx_st.append(NO_LEAVES)
                first.append(-1)
                flat += [NO_LEAVES] * len(per)
                continue
            bad = [j for j, st in enumerate(lanes) if st != bc.OK]
            tx_st.append(lanes[bad[0]] if bad else bc.OK)
            first.append(bad[0] if bad else -1)
            flat += lanes
        return tx_st, first, flat

    def check(self, got, rsa_on):
        ids, tx_st, first, sig_st = got[:4]
        w_tx, w_first, w_flat = self.want(rsa_on)
        assert [int(x) for x in sig_st] == w_flat
        assert [int(x) for x in tx_st] == w_tx
        assert [int(x) for x in first] == w_first
        for t, i in enumerate(self.ids):
            if i is not None:
                assert ids[t].tobytes() == i, t


@pytest.fixture(scope="module")
def batch(oracle):
    return Batch(oracle)


@pytest.fixture(params=["default", "3"])
def sliced(request, monkeypatch):
    """CORDAHIP_TX_SLICES unset / 3, and 7-signature chunks: transactions straddle chunk edges with their
    RSA lane on either side"""
    if request.param == "default":
        monkeypatch.delenv("CORDAHIP_TX_SLICES", raising=False)
    else:
        monkeypatch.setenv("CORDAHIP_TX_SLICES", request.param)
    monkeypatch.setenv("CORDAHIP_TX_SIG_CHUNK", "7")
    return request.param


def test_batch_has_rsa_lanes_on_both_sides_of_chunk_edges(batch):
    """with 7-signature chunks: an RSA lane last in a chunk, first in a chunk, and transactions that
    straddle an edge with the RSA lane before and after it"""
    pos, edge_before, edge_after, k = {}, 0, 0, 0
    for t, per in enumerate(batch.sigs):
        for j, x in enumerate(per):
            pos[(t, j)] = k
            k += 1
    for t, per in enumerate(batch.sigs):
        if len(per) < 2 or pos[(t, 0)] // 7 == pos[(t, len(per) - 1)] // 7:
            continue  # not straddling
        first_chunk = pos[(t, 0)] // 7
        for j, x in enumerate(per):
            if x[0] == RSA:
                if pos[(t, j)] // 7 == first_chunk:
                    edge_before += 1
                else:
                    edge_after += 1
    assert edge_before >= 1 and edge_after >= 1, (edge_before, edge_after)
    assert len(batch.rsa_lanes()) >= 30


def test_switch_off_rsa_lanes_unsupported(eng, batch, sliced):
    eng.set_rsa_on_device(False)
    batch.check(eng.signed_tx_verify(batch.txs, batch.sigs), rsa_on=False)
    flat = [x for per in batch.sigs for x in per]
    assert sum(x[0] == RSA for x in flat) >= 30


def test_switch_on_equals_model(eng, batch, sliced):
    eng.set_rsa_on_device(True)
    try:
        batch.check(eng.signed_tx_verify(batch.txs, batch.sigs), rsa_on=True)
        w_tx, w_first, _ = batch.want(True)
        assert (w_tx[3], w_first[3]) == (bc.BAD_SIG, 1) and (w_tx[10], w_first[10]) == (bc.BAD_SIG, 0)
        assert w_tx[8] == bc.BAD_KEY and w_tx[14] == bc.EMPTY and w_tx[20] == NO_LEAVES and w_tx[30] == NO_SIGS
        assert sum(x == bc.OK for x in w_tx) >= 25
    finally:
        eng.set_rsa_on_device(False)


def test_equals_generic_batch_with_flag(eng, batch):
    """an RSA lane of a signed transaction gets exactly the status cordahip_sig_verify with
    CORDAHIP_FLAG_RSA_ON_DEVICE and flags 0 gives for the same key, signature and the id as message"""
    lanes = [(t, j) for t, j in batch.rsa_lanes() if batch.ids[t] is not None]
    st, _ = eng.verify_batch([RSA] * len(lanes), [batch.sigs[t][j][1] for t, j in lanes],
                             [batch.sigs[t][j][2] for t, j in lanes], [batch.ids[t] for t, _ in lanes], rsa=True)
    assert [int(x) for x in st] == [batch.lane[t][j] for t, j in lanes]


def test_covered_call_required_key_is_the_rsa_key(eng, batch, sliced):
    """every transaction requires the notary's RSA key: with the switch on, coverage is evaluated over
    transactions whose RSA lanes verified"""
    from corda_amd import cover as C
    der = batch.notary["der"]
    must = [[(RSA, der)] for _ in batch.txs]
    eng.set_rsa_on_device(True)
    try:
        cov = C.flatten(must, batch.sigs)
        ids, tx_st, first, sig_st, req_st, first_missing = eng.signed_tx_verify_covered(batch.txs, batch.sigs, cov)
        w_tx, w_first, w_flat = batch.want(True)
        assert [int(x) for x in sig_st] == w_flat and [int(x) for x in first] == w_first
        signed_by_notary = [any(x[0] == RSA and x[1] == der for x in per) for per in batch.sigs]
        for t, w in enumerate(w_tx):
            if w != bc.OK:
                assert int(tx_st[t]) == w, t
            else:
                assert int(tx_st[t]) == (bc.OK if signed_by_notary[t] else _lib.TX_SIGNATURES_MISSING), t
        assert sum(int(x) == bc.OK for x in tx_st) >= 8
        assert sum(int(x) == _lib.TX_SIGNATURES_MISSING for x in tx_st) >= 8
    finally:
        eng.set_rsa_on_device(False)


def test_two_tickets_in_flight_waited_in_reverse(eng, batch, sliced):
    """both tickets carry RSA lanes; the second is the batch's first 28 transactions"""
    eng.set_rsa_on_device(True)
    try:
        t1 = eng.signed_tx_verify(batch.txs, batch.sigs, async_=True)
        t2 = eng.signed_tx_verify(batch.txs[:28], batch.sigs[:28], async_=True)
        r2 = t2.wait()
        r1 = t1.wait()
        batch.check(r1, rsa_on=True)
        w_tx, w_first, w_flat = batch.want(True)
        n28 = sum(len(per) for per in batch.sigs[:28])
        assert n28 < len(w_flat) and [int(x) for x in r2[3]] == w_flat[:n28]
        assert [int(x) for x in r2[1]] == w_tx[:28] and [int(x) for x in r2[2]] == w_first[:28]
    finally:
        eng.set_rsa_on_device(False)


def test_routed_to_the_registered_notary_key(eng, batch, sliced):
    """the same batch with cordahip_vkey_set_routing_rsa on and the notary's key registered: identical
    outputs, keyed stats equal to that key's rows that reached the device"""
    der = batch.notary["der"]
    kl = (batch.notary["n"].bit_length() + 7) // 8
    device_rows = [(t, j) for t, j in batch.rsa_lanes()
                   if not isinstance(bc.decode_key(batch.sigs[t][j][1]), int) and 0 < len(batch.sigs[t][j][2]) <=
                   (bc.decode_key(batch.sigs[t][j][1])[0].bit_length() + 7) // 8]
    keyed = sum(batch.sigs[t][j][1] == der and len(batch.sigs[t][j][2]) <= kl for t, j in device_rows)
    kid, st = eng.vkey_add_rsa(der)
    assert st == bc.OK
    eng.set_rsa_on_device(True)
    eng.vkey_set_routing_rsa(True)
    try:
        before = eng.vkey_route_stats_rsa()
        batch.check(eng.signed_tx_verify(batch.txs, batch.sigs), rsa_on=True)
        after = eng.vkey_route_stats_rsa()
        assert (after[0] - before[0], after[1] - before[1]) == (keyed, len(device_rows) - keyed)
        assert keyed >= 12 and len(device_rows) - keyed >= 8
    finally:
        eng.vkey_set_routing_rsa(False)
        eng.set_rsa_on_device(False)
        eng.vkey_remove(kid)


def test_txcomp_call(eng, oracle):
    """a component batch: the GPU writes the leaves, then the same signature pipeline"""
    from corda_amd.corpus import cash_issue_items
    rng = np.random.default_rng(5)
    prng = random.Random(0x7C)
    ntx = 12
    blob, items, _ = cash_issue_items(rng.integers(0, 256, (ntx, 32), dtype=np.uint8),
                                      rng.integers(0, 256, (ntx, 32), dtype=np.uint8), bytes(range(32)),
                                      rng.integers(1, 10**9, ntx), rng.integers(-2**63, 2**63 - 1, ntx))
    it = items.reshape(-1).copy()
    host_it = it.copy()
    host_it["data"] += np.uint64(blob.ctypes.data)
    hb, ho = _lib.kryo_encode_array(host_it)
    leaves = [[hb[int(ho[5 * t + j]):int(ho[5 * t + j + 1])].tobytes() for j in range(5)] for t in range(ntx)]
    ids = [oracle_id(oracle, leaves[t]) for t in range(ntx)]
    k = load_keys()["openssl_3072"]
    sigs, lane = [], []
    for t in range(ntx):
        pub, sg = ed_sign(oracle, hashlib.sha256(b"tc%d" % t).digest(), ids[t])
        rs = rsa_sign(prng, k, ids[t])
        if t % 4 == 1:
            rs = rs[:9] + bytes([rs[9] ^ 1]) + rs[10:]
        sigs.append([(ED, pub, sg), (RSA, k["der"], rs)])
        lane.append([bc.OK, bc.verify(k["der"], rs, ids[t])])
    tio = np.arange(0, 5 * ntx + 1, 5, dtype=np.uint64)
    for on in (False, True):
        eng.set_rsa_on_device(on)
        try:
            got_ids, tx_st, first, sig_st = eng.signed_txcomp_verify_arrays(blob, it, tio, sigs)
        finally:
            eng.set_rsa_on_device(False)
        want = [st if on else bc.UNSUPPORTED for _, st in lane]
        assert [int(x) for x in sig_st[1::2]] == want and [int(x) for x in sig_st[0::2]] == [bc.OK] * ntx
        assert [int(x) for x in tx_st] == want
        assert [int(x) for x in first] == [-1 if w == bc.OK else 1 for w in want]
        assert all(got_ids[t].tobytes() == ids[t] for t in range(ntx))
    assert bc.BAD_SIG in [st for _, st in lane] and bc.OK in [st for _, st in lane]


def test_verify_signatures_batch_flow(eng, oracle):
    """resolve.verify_signatures_batch: nothing raised for a valid RSA-signed transaction with the switch
    on; with it off the same call reports the UNSUPPORTED lane's IllegalArgumentException"""
    from corda_amd import resolve
    rng = random.Random(0x7D)
    k = load_keys()["openssl_2048"]
    comps = [rng.randbytes(n) for n in (70, 31, 45)]
    tid = oracle_id(oracle, comps)
    pub, sg = ed_sign(oracle, hashlib.sha256(b"flow").digest(), tid)
    stx = resolve.SignedTx(comps, [(ED, pub, sg), (RSA, k["der"], rsa_sign(rng, k, tid))], must_sign=[pub, k["der"]])
    eng.set_rsa_on_device(True)
    try:
        out = resolve.verify_signatures_batch(eng, [stx])
        assert out[0].error is None and out[0].id == tid
    finally:
        eng.set_rsa_on_device(False)
    out = resolve.verify_signatures_batch(eng, [stx])
    assert isinstance(out[0].error, resolve.IllegalArgumentException) and out[0].first_bad_sig == 1
    assert "Unsupported" in str(out[0].error)
