"""resolve.notarise_transactions (K22: components -> ids -> signatures -> inputs and window ->
commit -> notary signature on one stream) against the serial model
resolve.commit_input_states over the refs and windows the test built the transactions from,
gated by the oracle's signature verdicts, plus the oracle's Ed25519 verify of every signature
the notary returns. One batch holds fresh payments, a double spend inside the batch, a
resubmitted transaction, a bad owner signature, a window outside tolerance and an issue; a
second batch then runs against the log the first one left."""
import hashlib

import numpy as np
import pytest

import kryo_notary_model as N
import kryo_payment_model as M
from corda_amd import _lib, resolve
from corda_amd.corpus import (CASH_ISSUE_COMMAND, KRYO_IDS, TRANSACTION_TYPE_GENERAL, cash_payment_items, x500_name)
from test_gpu_kryo_payment import NOTARY_SEED, _keypairs
from test_gpu_txcomp import _oracle_id, _sign

pytestmark = pytest.mark.gpu
NOW_S = 1500000000
NOW, TOLERANCE = NOW_S * 10**9, 60 * 10**9


def _tx(oracle, comps, signer_seeds, refs, window, corrupt=False):
    """(components, sigs), id, refs, window in ns -- signed by signer_seeds over the model's id"""
    txid = _oracle_id(oracle, [M.component_leaf(*c) for c in comps])
    sigs = [(_sign(oracle, s, b"")[0], _sign(oracle, s, txid)[1]) for s in signer_seeds]
    if corrupt:
        g = bytearray(sigs[-1][1])
        g[9] ^= 4
        sigs[-1] = (sigs[-1][0], bytes(g))
    w = None if window is None else (None if window[0] is None else N.instant_ns(window[0]),
                                     None if window[1] is None else N.instant_ns(window[1]))
    return {"stx": (comps, sigs), "id": txid, "refs": refs, "window": w, "bad_sig": corrupt}


def _payments(oracle, seeds, pubs, notary_pub, ntx, seed):
    c = cash_payment_items(pubs, notary_pub, ntx, seed, window_frac=0.4, now_s=NOW_S, with_components=True)
    return [_tx(oracle, c["components"][t], [seeds[o] for o in c["signers"][t]], c["refs"][t], c["windows"][t])
            for t in range(ntx)]


def _variant(oracle, tx, seeds_of, **kw):
    """tx with another output quantity (another id) -- and what kw changes"""
    comps = [(k, dict(v, quantity=v["quantity"] + 1), c) if k == "cash_state" else (k, v, c) for k, v, c in tx["stx"][0]]
    window = kw.pop("window", "same")
    if window != "same":
        comps = [c for c in comps if c[0] != "time_window"] + [("time_window", _lib.pack_time_window(*window), 0)]
    else:
        tw = [c for c in comps if c[0] == "time_window"]
        window = M._window(tw[0][1]) if tw else None
    return _tx(oracle, comps, seeds_of, tx["refs"], window, **kw)


def _issue(oracle, seed, owner_pub, notary_pub):
    ed, x5 = KRYO_IDS["ed25519_key"], KRYO_IDS["x500_name"]
    issuer = _sign(oracle, seed, b"")[0]
    notary = x500_name("Notary Service", "Zurich", "CH")
    d = {"issuer": (x500_name("Bank A", "London", "GB"), issuer, ed), "reference": b"\x01", "owner": (b"", owner_pub, ed),
         "notary": (notary, notary_pub, ed), "currency": "USD", "digits": 2,
         "legal_ref": hashlib.sha256(b"https://www.big-book-of-banking-law.gov/cash-claims.html").digest(),
         "encumbrance": None, "quantity": 12345}
    comps = [("cash_state", d, x5), ("issue_command", (CASH_ISSUE_COMMAND, 77, [(ed, issuer)]), KRYO_IDS["arrays_as_list"]),
             ("party", (notary, notary_pub, ed), x5), ("ed25519_key", issuer, ed),
             ("kotlin_object", TRANSACTION_TYPE_GENERAL, 0)]
    return _tx(oracle, comps, [seed], [], None)


def _check(engine, oracle, log_id, model_log, key_id, notary_pub, txs, callers):
    detail = {}
    answers, rows = resolve.notarise_transactions(engine, log_id, [t["stx"] for t in txs], callers, key_id, NOW,
                                                  TOLERANCE, detail=detail)
    gate = [1 if t["bad_sig"] else 0 for t in txs]
    want = resolve.commit_input_states(model_log, [(t["id"], callers[i], t["refs"], t["window"])
                                                   for i, t in enumerate(txs)], NOW, TOLERANCE, gate=gate)
    w_status, w_committed, w_state, w_by = want
    assert [x.tobytes() for x in detail["ids"]] == [t["id"] for t in txs]
    assert detail["committed"].tolist() == w_committed
    # the extracted rows are the transactions' inputs (a gated transaction keeps its rows: it is skipped by the commit)
    off = detail["tx_ref_off"].tolist()
    for i, t in enumerate(txs):
        got = [(r[:32].tobytes(), int.from_bytes(r[32:].tobytes(), "little")) for r in detail["refs"][off[i]:off[i + 1]]]
        assert got == [(bytes(h), ix) for h, ix in t["refs"]], i
    want_rows = []
    for i, t in enumerate(txs):
        st, a = w_status[i], answers[i]
        if gate[i]:
            assert detail["status"][i] == resolve.BAD_SIG and isinstance(a, resolve.NotaryError)
            assert a.kind == "TransactionInvalid" and a.tx_id == t["id"]
        elif st == 17:
            assert detail["status"][i] == 17 and a == resolve.NotaryError("TimeWindowInvalid", t["id"])
        elif st == 16:
            hist = {}
            for r, by in zip(t["refs"], w_by[i]):
                if by is not None:
                    hist.setdefault((bytes(r[0]), int(r[1])), by)
            assert detail["status"][i] == 16 and a == resolve.NotaryError("Conflict", t["id"], hist) and hist
        else:
            assert st == 0 and detail["status"][i] == 0 and isinstance(a, bytes) and len(a) == 64
            assert oracle.oracle_ed25519_verify(notary_pub, 32, a, 64, t["id"], 32) == 0, i
        if w_committed[i]:
            want_rows += [((bytes(h), ix), (t["id"], k, callers[i])) for k, (h, ix) in enumerate(t["refs"])]
    assert sorted(rows) == sorted(want_rows)
    return w_status, w_committed


def test_notarise_transactions_two_batches(engine, oracle):
    seeds, pubs = _keypairs(oracle, 16)
    key_id, notary_pub = engine.signer_add_ed25519(NOTARY_SEED)
    log_id = engine.commit_log_create(10)
    try:
        pay = _payments(oracle, seeds, pubs, notary_pub, 14, 77)
        assert any(t["window"] is not None for t in pay[:10])  # valid windows among the fresh payments
        signers_of = lambda t: [s for s in seeds if _sign(oracle, s, b"")[0] in [k for k, _ in t["stx"][1]]]  # noqa: E731
        batch1 = pay[:10] + [
            _variant(oracle, pay[2], signers_of(pay[2])),                       # a double spend inside the batch
            pay[4],                                                             # resubmitted: committed = 0, signed again
            _variant(oracle, pay[10], signers_of(pay[10]), corrupt=True),       # a bad owner signature
            _variant(oracle, pay[11], signers_of(pay[11]), window=(None, (NOW_S - 3600, 0))),  # a window outside tolerance
            _issue(oracle, hashlib.sha256(b"issuer").digest(), pubs[0].tobytes(), notary_pub),
        ]
        callers1 = [7 + (i % 3) for i in range(10)] + [9, 7 + (4 % 3), 3, 3, 5]
        model_log = {}
        st, cm = _check(engine, oracle, log_id, model_log, key_id, notary_pub, batch1, callers1)
        assert st[:10] == [0] * 10 and cm[:10] == [1] * 10
        assert st[10] == 16 and (st[11], cm[11]) == (0, 0) and cm[12] == 0 and st[13] == 17 and (st[14], cm[14]) == (0, 1)
        # the second batch against the log the first one left: the spent inputs conflict, the skipped
        # and the out-of-window transactions' inputs are still free, a resubmission is signed again
        batch2 = [pay[10], pay[11], pay[12], pay[13], _variant(oracle, pay[0], signers_of(pay[0])), pay[1], batch1[10]]
        callers2 = [1, 2, 3, 4, 5, callers1[1], 9]
        st, cm = _check(engine, oracle, log_id, model_log, key_id, notary_pub, batch2, callers2)
        assert cm[:4] == [1, 1, 1, 1] and st[4] == 16 and (st[5], cm[5]) == (0, 0) and st[6] == 16
        entries, _, _ = engine.commit_log_stats(log_id)
        assert entries == len(model_log)
    finally:
        engine.commit_log_destroy(log_id)
        engine.signer_remove(key_id)
