"""resolve.notarise_transactions with (scheme, key, sig) triples (K23): payments signed by Ed25519,
P-256 and RSA parties in one batch go through the mixed device call on one stream. Answers,
committed rows and conflicts equal the same batch through the host-memory call
(Engine.signed_txcomp_verify, RSA on the device) plus the serial model resolve.commit_input_states;
the notary's signatures verify under the oracle, with an Ed25519 and with a P-256 notary key."""
import hashlib
import random

import pytest

import bc_ecdsa as ec
from corda_amd import resolve
from test_gpu_kryo_payment import NOTARY_SEED, _keypairs
from test_gpu_notarise_transactions import NOW, TOLERANCE, _payments, _variant
from test_gpu_rsa_route import by_class, load_keys
from test_gpu_rsa_route import sign as rsa_sign
from test_gpu_txcomp import _sign

pytestmark = pytest.mark.gpu
ED, R1, RSA = 4, 3, 1


def _mixed(txs):
    """the payments' Ed25519 owner signatures as triples, plus a P-256 or an RSA party's over the id"""
    rng = random.Random(29)
    rsa_keys = [by_class(load_keys(), w)[0] for w in (64, 96, 128)]
    out = []
    for t, tx in enumerate(txs):
        comps, pairs = tx["stx"]
        sigs = [(ED, k, g) for k, g in pairs]
        if t % 3 == 1:
            d = 1000 + t
            rr, ss = ec.sign(R1, d, tx["id"], rng.randrange(1, ec.CURVES[R1].n))
            pk = ec.keypair(R1, d)
            sigs.append((R1, ec.compress(pk) if t % 2 else pk, ec.der_encode(rr, ss)))
        if t % 3 == 2:
            k = rsa_keys[t % 3 if t % 2 else 0]
            sigs.insert(0, (RSA, k["der"], rsa_sign(rng, k, tx["id"])))
        out.append(dict(tx, stx=(comps, sigs)))
    return out


def _spoil(tx, which):
    """a bit of the tx's signature of scheme `which` flipped"""
    comps, sigs = tx["stx"]
    q = [i for i, x in enumerate(sigs) if x[0] == which][0]
    g = bytearray(sigs[q][2])
    g[len(g) - 3] ^= 8
    sigs = list(sigs)
    sigs[q] = (sigs[q][0], sigs[q][1], bytes(g))
    return dict(tx, stx=(comps, sigs))


def _check(engine, oracle, log_id, model_log, key_id, family, verify_answer, txs, callers):
    detail = {}
    answers, rows = resolve.notarise_transactions(engine, log_id, [t["stx"] for t in txs], callers, key_id, NOW,
                                                  TOLERANCE, detail=detail, notary_family=family)
    # the host-memory reference of the verify step, then the serial model of the commit
    ids, tx_status, _, _ = engine.signed_txcomp_verify([t["stx"][0] for t in txs], [t["stx"][1] for t in txs])
    assert [x.tobytes() for x in ids] == [t["id"] for t in txs] == [x.tobytes() for x in detail["ids"]]
    assert detail["verify_status"].tolist() == [int(x) for x in tx_status]
    gate = [int(x != 0) for x in tx_status]
    w_status, w_committed, _, w_by = resolve.commit_input_states(
        model_log, [(t["id"], callers[i], t["refs"], t["window"]) for i, t in enumerate(txs)], NOW, TOLERANCE, gate=gate)
    assert detail["committed"].tolist() == w_committed
    want_rows = []
    for i, t in enumerate(txs):
        a = answers[i]
        if gate[i]:
            assert a == resolve.NotaryError("TransactionInvalid", t["id"]) and detail["status"][i] == tx_status[i]
        elif w_status[i] == 17:
            assert a == resolve.NotaryError("TimeWindowInvalid", t["id"])
        elif w_status[i] == 16:
            hist = {}
            for r, by in zip(t["refs"], w_by[i]):
                if by is not None:
                    hist.setdefault((bytes(r[0]), int(r[1])), by)
            assert a == resolve.NotaryError("Conflict", t["id"], hist) and hist
        else:
            assert w_status[i] == 0 and isinstance(a, bytes) and verify_answer(a, t["id"]), i
        if w_committed[i]:
            want_rows += [((bytes(h), ix), (t["id"], k, callers[i])) for k, (h, ix) in enumerate(t["refs"])]
    assert sorted(rows) == sorted(want_rows)
    return gate, w_status, w_committed


def test_notarise_mixed_schemes_ed25519_and_ecdsa_notary(engine, oracle):
    seeds, pubs = _keypairs(oracle, 16)
    ed_id, notary_pub = engine.signer_add_ed25519(NOTARY_SEED)
    ec_id, st, ec_pub = engine.signer_add_ecdsa(R1, hashlib.sha256(b"p256 notary").digest())
    assert st == 0
    log_id = engine.commit_log_create(10)
    engine.set_rsa_on_device(True)
    try:
        pay = _payments(oracle, seeds, pubs, notary_pub, 16, 91)
        signers_of = lambda t: [s for s in seeds if _sign(oracle, s, b"")[0] in [k for k, _ in t["stx"][1]]]  # noqa: E731
        plain = pay[:12] + [_variant(oracle, pay[2], signers_of(pay[2]))]  # the last: a double spend in the batch
        mixed = _mixed(plain)
        assert {x[0] for t in mixed for x in t["stx"][1]} == {ED, R1, RSA}
        batch1 = mixed[:10] + [mixed[12], _spoil(mixed[10], R1), _spoil(mixed[11], RSA)]
        callers1 = [3 + i % 4 for i in range(len(batch1))]
        model_log = {}
        ed_ok = lambda a, txid: len(a) == 64 and oracle.oracle_ed25519_verify(notary_pub, 32, a, 64, txid, 32) == 0  # noqa: E731
        gate, st1, cm1 = _check(engine, oracle, log_id, model_log, ed_id, "ed25519", ed_ok, batch1, callers1)
        assert gate == [0] * 11 + [1, 1] and cm1[:10] == [1] * 10 and st1[10] == 16 and cm1[11:] == [0, 0]
        # a second batch against the log the first left, answered with the P-256 notary key: the
        # transactions whose signatures were spoilt now pass, a spent input conflicts, one is resubmitted
        batch2 = [mixed[10], mixed[11], mixed[12], mixed[4]] + _mixed(pay[12:16])
        callers2 = [1, 2, 3, callers1[4], 5, 6, 7, 8]
        ec_ok = lambda a, txid: oracle.oracle_ecdsa_verify(R1, ec_pub, 65, a, len(a), txid, 32) == 0  # noqa: E731
        gate, st2, cm2 = _check(engine, oracle, log_id, model_log, ec_id, "ecdsa", ec_ok, batch2, callers2)
        assert gate == [0] * 8 and cm2[:2] == [1, 1] and st2[2] == 16 and (st2[3], cm2[3]) == (0, 0) and cm2[4:] == [1] * 4
        entries, _, _ = engine.commit_log_stats(log_id)
        assert entries == len(model_log)
    finally:
        engine.set_rsa_on_device(False)
        engine.commit_log_destroy(log_id)
        engine.signer_remove(ed_id)
        engine.signer_remove(ec_id)
