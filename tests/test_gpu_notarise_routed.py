"""resolve.notarise_transactions with registered-key routing inside its mixed verify step (K24) and
with an RSA notary key: payments signed by Ed25519, P-256 and RSA parties whose keys are registered
answer and commit exactly as with routing off, the route counters of all three families move, and a
notary_family="rsa" run returns RSASSA-PSS signatures under the caller's salts -- the bytes the
Python model (tests/golden/bc_rsa_pss.py) and Engine.rsa_sign_batch give for the same ids."""
import hashlib

import pytest

import bc_ecdsa as ec
import bc_rsa_pss as bc
from corda_amd import resolve
from test_gpu_kryo_payment import NOTARY_SEED, _keypairs
from test_gpu_notarise_mixed import ED, R1, RSA, _mixed, _spoil
from test_gpu_notarise_transactions import NOW, TOLERANCE, _payments
from test_gpu_rsa_route import by_class, load_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    """a context of this module's own: its registries and its counters"""
    from corda_amd.engine import Engine
    with Engine(1) as e:
        yield e


@pytest.fixture(scope="module")
def batch(eng, oracle):
    seeds, pubs = _keypairs(oracle, 16)
    kid, notary_pub = eng.signer_add_ed25519(NOTARY_SEED)  # for its public key, the payments' notary field
    eng.signer_remove(kid)
    pay = _payments(oracle, seeds, pubs, notary_pub, 12, 93)
    mixed = _mixed(pay)
    assert {x[0] for t in mixed for x in t["stx"][1]} == {ED, R1, RSA}
    return mixed[:10] + [_spoil(mixed[10], R1), _spoil(mixed[11], RSA)]


def _switches(e, on):
    e.vkey_set_routing(on)
    e.vkey_set_routing_ecdsa(on)
    e.vkey_set_routing_rsa(on)
    e.vkey_set_routing_device(on)


def _stats(e):
    return e.vkey_route_stats(), e.vkey_route_stats_ecdsa(), e.vkey_route_stats_rsa()


def test_notarise_routed_equals_unrouted(eng, oracle, batch):
    callers = [3 + i % 4 for i in range(len(batch))]
    ed_id, _ = eng.signer_add_ed25519(NOTARY_SEED)
    logs = [eng.commit_log_create(10), eng.commit_log_create(10)]  # equal state for the two runs
    flat = [x for t in batch for x in t["stx"][1]]
    kids = []
    eng.set_rsa_on_device(True)
    try:
        # every party's key registered: the Ed25519 owners, the P-256 parties, the RSA parties
        for key in sorted({x[1] for x in flat if x[0] == ED}):
            kids.append(eng.vkey_add_ed25519(key)[0])
        for t in range(len(batch)):  # test_gpu_notarise_mixed._mixed: transaction t's P-256 party
            if t % 3 == 1:
                kids.append(eng.vkey_add_ecdsa(R1, ec.keypair(R1, 1000 + t))[0])
        for der in sorted({x[1] for x in flat if x[0] == RSA}):
            kids.append(eng.vkey_add_rsa(der)[0])
        runs = []
        for on, log_id in zip((False, True), logs):
            _switches(eng, on)
            b0 = _stats(eng)
            detail = {}
            answers, rows = resolve.notarise_transactions(eng, log_id, [t["stx"] for t in batch], callers, ed_id, NOW,
                                                          TOLERANCE, detail=detail)
            mv = tuple((a[0] - b[0], a[1] - b[1]) for b, a in zip(b0, _stats(eng)))
            runs.append((answers, sorted(rows), {k: v.tolist() for k, v in detail.items()}, mv))
        off, on = runs
        assert on[0] == off[0] and on[1] == off[1] and on[2] == off[2]
        assert sum(isinstance(a, bytes) for a in on[0]) >= 8 and on[2]["verify_status"][-2:] != [0, 0]
        assert off[3] == ((0, 0),) * 3
        n_of = lambda sch: sum(x[0] == sch for x in flat)  # noqa: E731 (every lane's key is registered)
        assert on[3] == ((n_of(ED), 0), (n_of(R1), 0), (n_of(RSA), 0)), on[3]
    finally:
        _switches(eng, False)
        eng.set_rsa_on_device(False)
        for kid in kids:
            eng.vkey_remove(kid)
        for log_id in logs:
            eng.commit_log_destroy(log_id)
        eng.signer_remove(ed_id)


def test_notarise_with_an_rsa_notary_key(eng, oracle, batch):
    k = by_class(load_keys(), 96)[0]
    p, q, d = k["p"], k["q"], k["d"]
    kid, st, mod = eng.signer_add_rsa(p, q, d % (p - 1), d % (q - 1), pow(q, -1, p), k["e"])
    assert st == 0 and int.from_bytes(mod, "big") == k["n"]
    callers = [1 + i % 3 for i in range(len(batch))]
    salts = [hashlib.sha256(b"notary salt %d" % t).digest() for t in range(len(batch))]
    log_id = eng.commit_log_create(10)
    eng.set_rsa_on_device(True)
    try:
        stxs = [t["stx"] for t in batch]
        with pytest.raises(AssertionError):
            resolve.notarise_transactions(eng, log_id, stxs, callers, kid, NOW, TOLERANCE, notary_family="rsa")
        with pytest.raises(AssertionError):
            resolve.notarise_transactions(eng, log_id, stxs, callers, kid, NOW, TOLERANCE, salts=salts)
        with pytest.raises(AssertionError):
            resolve.notarise_transactions(eng, log_id, stxs, callers, kid, NOW, TOLERANCE, notary_family="ecdsa",
                                          salts=salts)
        assert eng.commit_log_stats(log_id)[0] == 0  # nothing was committed by the refused calls
        detail = {}
        answers, rows = resolve.notarise_transactions(eng, log_id, stxs, callers, kid, NOW, TOLERANCE, detail=detail,
                                                      notary_family="rsa", salts=salts)
        ids = [t["id"] for t in batch]
        assert [x.tobytes() for x in detail["ids"]] == ids
        host_sig, host_len, host_st = eng.rsa_sign_batch([kid] * len(ids), ids, salts)
        signed = [t for t, a in enumerate(answers) if isinstance(a, bytes)]
        assert len(signed) >= 8 and all(detail["status"][t] == 0 for t in signed)
        klen = (k["n"].bit_length() + 7) // 8
        for t in signed:
            a = answers[t]
            assert len(a) == klen and bc.verify(k["der"], a, ids[t]) == bc.OK
            em = bc.encode_em(ids[t], k["n"].bit_length(), salts[t])  # the signature under the given salt
            assert a == bc.sign_crt(em, p, q, d).to_bytes(klen, "big")
            assert host_st[t] == 0 and a == host_sig[t, :int(host_len[t])].tobytes()
        # gated by the commit status: the two transactions whose signatures were spoilt are not signed
        for t in (len(batch) - 2, len(batch) - 1):
            assert answers[t] == resolve.NotaryError("TransactionInvalid", ids[t])
        assert rows
    finally:
        eng.set_rsa_on_device(False)
        eng.commit_log_destroy(log_id)
        eng.signer_remove(kid)
