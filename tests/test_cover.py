"""Required-signer coverage on the host: cordahip_cover_eval_host (the evaluator
of corda_amd/csrc/cover_core.hpp, which the GPU kernel and the covered
signed-tx calls also run) against the Python rule of corda_amd/resolve.py.

Reference behaviour followed:
  SignedTransaction.verifySignatures / getMissingSignatures   SignedTransaction.kt:70-85, :102-108
  CompositeKey.isFulfilledBy / checkFulfilledBy                CompositeKey.kt:186-209
  CompositeKey.checkValidity / checkConstraints / totalWeight  CompositeKey.kt:73-85, :110-133
  the cases of CompositeKeyTests.kt:42-221, :284-305

The Python side keeps keys as (scheme, bytes) pairs, so resolve.is_fulfilled_by's
`key in keys` is scheme-and-byte equality, the wire form's leaf rule.
"""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from corda_amd import _lib
from corda_amd import cover as C
from corda_amd import resolve as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RSA, K1, R1, ED, SPHINCS = 1, 2, 3, 4, 5
OK, NO_SIGS, MISSING_TX, BAD_COVER = 0, _lib.TX_NO_SIGNATURES, _lib.TX_SIGNATURES_MISSING, _lib.TX_BAD_COVER
FULFILLED, MISSING, ALLOWED, NOT_EVALUATED, MALFORMED = 0, 1, 2, 3, 4
INT_MAX = 2**31 - 1

CK = R.CompositeKey


def key(i, scheme=ED, n=32):
    return (scheme, bytes([i]) * n)


ALICE, BOB, CHARLIE = key(1), key(2), key(3)


def node(*children, threshold=None):
    """CompositeKey.Builder: addKey(node, weight) ... build(threshold = total weight)."""
    ch = tuple(c if isinstance(c, tuple) and isinstance(c[1], int) and not isinstance(c[0], int) else (c, 1)
               for c in children)
    return CK(sum(w for _, w in ch) if threshold is None else threshold, ch)


def w(n, weight):
    return (n, weight)


# ---- the Python rule ------------------------------------------------------------
def py_valid(k):
    """checkValidity -> checkConstraints on every node (CompositeKey.kt:73-85, :110-133),
    without the duplicate-children test (not part of the wire form's contract)."""
    if not isinstance(k, CK):
        return True
    if len(k.children) < 2 or not 0 < k.threshold <= INT_MAX:
        return False
    total = 0
    for ch, wt in k.children:
        if not 0 < wt <= INT_MAX:
            return False
        total += wt
        if total > INT_MAX:
            return False
    return k.threshold <= total and all(py_valid(ch) for ch, _ in k.children)


def py_tx(status, must_sign, sig_keys, allowed):
    """One transaction by the header's order: (tx_status, [req_status], first_missing)."""
    if status != OK:
        return status, [NOT_EVALUATED] * len(must_sign), -1
    keys = set(sig_keys)
    req = []
    for k in must_sign:
        if not py_valid(k):
            req.append(MALFORMED)
        elif R.is_fulfilled_by(k, keys):
            req.append(FULFILLED)
        else:
            req.append(ALLOWED if k in allowed else MISSING)
    if MALFORMED in req:
        return BAD_COVER, req, req.index(MALFORMED)
    if MISSING in req:
        return MISSING_TX, req, req.index(MISSING)
    return OK, req, -1


def run(must_sign, sig_keys, status=None, allowed=()):
    """cover_eval_host over a batch: must_sign[t], sig_keys[t] = [(scheme, key)]."""
    cov = C.flatten(must_sign, None, allowed)
    status = [OK] * len(must_sign) if status is None else status
    st, req, fm = C.cover_eval_host(cov, status, sig_keys)
    off = cov.tx_req_off
    return [(int(st[t]), [int(x) for x in req[int(off[t]):int(off[t + 1])]], int(fm[t]))
            for t in range(len(must_sign))], cov


def check_against_rule(must_sign, sig_keys, status=None, allowed=()):
    got, cov = run(must_sign, sig_keys, status, allowed)
    status = [OK] * len(must_sign) if status is None else status
    want = [py_tx(status[t], must_sign[t], sig_keys[t], set(allowed)) for t in range(len(must_sign))]
    assert got == want
    return got, cov


# ---- CompositeKeyTests.kt --------------------------------------------------------
def subsets(keys):
    return [[k for i, k in enumerate(keys) if m >> i & 1] for m in range(1 << len(keys))]


def test_composite_key_tests_cases():
    alice_or_bob = node(ALICE, BOB, threshold=1)                      # :48-54
    alice_and_bob = node(ALICE, BOB)                                  # :57-69
    ab_or_c = node(alice_and_bob, CHARLIE, threshold=1)               # :72-80
    weighted = node(w(node(w(ALICE, 2), w(BOB, 1), threshold=2), 3), w(CHARLIE, 2), threshold=3)  # :105-114
    node1, node2 = node(ALICE, BOB, threshold=1), node(ALICE, BOB, threshold=2)
    tree1 = node(w(node1, 13), w(node2, 27))                          # :125-131
    tree2 = node(w(node2, 27), w(node1, 13))
    tree1_any = node(w(node1, 13), w(node2, 27), threshold=27)
    two_of_three = node(ALICE, BOB, CHARLIE, threshold=2)             # :154-165
    trees = [ALICE, alice_or_bob, alice_and_bob, ab_or_c, weighted, tree1, tree2, tree1_any, two_of_three]
    cases = [(i, s) for i in range(len(trees)) for s in subsets([ALICE, BOB, CHARLIE])]
    got, _ = check_against_rule([[trees[i]] for i, _ in cases], [s for _, s in cases])
    verdict = {(i, tuple(s)): g[1][0] == FULFILLED for (i, s), g in zip(cases, got)}
    # the assertions CompositeKeyTests.kt itself makes
    assert verdict[0, (ALICE,)] and not verdict[0, (CHARLIE,)]
    assert verdict[1, (ALICE,)] and verdict[1, (BOB,)] and verdict[1, (ALICE, BOB)] and not verdict[1, (CHARLIE,)]
    assert verdict[2, (ALICE, BOB)] and not verdict[2, (ALICE,)] and not verdict[2, (BOB,)]
    assert verdict[3, (ALICE, BOB)] and verdict[3, (CHARLIE,)] and not verdict[3, (ALICE,)]
    assert not verdict[6, (ALICE,)] and verdict[5, (ALICE, BOB)] and verdict[7, (ALICE, BOB)]
    for s in subsets([ALICE, BOB, CHARLIE]):
        assert verdict[8, tuple(s)] == (len(s) >= 2)


def test_five_scheme_key():
    """CompositeKeyTests.kt:284-305: one key of every scheme, all required."""
    keys = [key(10, RSA, 270), key(11, K1, 33), key(12, R1, 65), key(13, ED, 32), key(14, SPHINCS, 1056)]
    ck = node(*keys)
    got, _ = check_against_rule([[ck], [ck]], [keys, keys[1:]])
    assert got[0][0] == OK and got[1] == (MISSING_TX, [MISSING], 0)


def nested_keys():
    key1 = node(ALICE, BOB)  # CompositeKeyTests.kt:215-221
    key2 = node(ALICE, key1)
    key3 = node(ALICE, key2)
    key4 = node(ALICE, key3)
    key5 = node(ALICE, key4)
    key6 = node(ALICE, key5, key2)
    return [key1, key2, key3, key4, key5, key6]


def test_nested_keys_depth():
    ks = nested_keys()
    must = [[k] for k in ks] * 3
    sigs = [[ALICE, BOB]] * 6 + [[ALICE]] * 6 + [[BOB]] * 6
    got, cov = check_against_rule(must, sigs)
    assert [g[0] for g in got] == [OK] * 6 + [MISSING_TX] * 12
    assert int(cov.req_tok_off[6] - cov.req_tok_off[5]) == 18  # key6: 10 leaves under 8 nodes


def test_deep_and_wide_trees_beyond_the_inline_stack():
    """Trees of more tokens than a host worker's inline stack (64 slots): a 300-leaf
    2-of-300 key, and a chain 200 nodes deep."""
    leaves = [key(i % 251 + 1, ED, 33 + i // 251) for i in range(300)]
    wide = node(*leaves, threshold=2)
    deep = node(ALICE, BOB)
    for _ in range(200):
        deep = node(CHARLIE, deep, threshold=1)
    deep_and = node(ALICE, BOB)
    for _ in range(200):
        deep_and = node(CHARLIE, deep_and)
    must = [[wide], [wide], [deep], [deep], [deep_and], [deep_and], [ALICE, wide, deep_and]]
    sigs = [[leaves[7], leaves[299]], [leaves[7]], [ALICE, BOB], [ALICE], [ALICE, BOB, CHARLIE], [ALICE, BOB],
            [ALICE, leaves[0], leaves[1]]]
    cov = C.flatten(must, None)
    st, req, fm = C.cover_eval_host(cov, [OK] * len(must), sigs)
    # (py_valid / is_fulfilled_by recurse: fine at these depths)
    want = [py_tx(OK, must[t], sigs[t], set()) for t in range(len(must))]
    assert [int(x) for x in st] == [x[0] for x in want] == [OK, MISSING_TX, OK, MISSING_TX, OK, MISSING_TX, MISSING_TX]
    assert [int(x) for x in req] == [r for x in want for r in x[1]]
    assert [int(x) for x in fm] == [x[2] for x in want]


# ---- seeded random transactions ---------------------------------------------------
def random_tree(rng, pool, depth):
    if depth == 0 or rng.random() < 0.45:
        return rng.choice(pool)
    n = rng.choice((2, 2, 3, 4))
    ch = tuple((random_tree(rng, pool, depth - 1), rng.choice((1, 1, 2, 5))) for _ in range(n))
    total = sum(x for _, x in ch)
    k = CK(rng.randint(1, total), ch)
    flaw = rng.random()
    if flaw < 0.02:
        k = CK(0, ch)
    elif flaw < 0.04:
        k = CK(total + 1, ch)
    elif flaw < 0.06:
        k = CK(k.threshold, ((ch[0][0], 0),) + ch[1:])
    elif flaw < 0.07:
        k = CK(1, ch[:1])
    return k


def random_batch(seed, ntx):
    rng = random.Random(seed)
    pool = [key(i, ED) for i in range(1, 9)] + [key(20, K1, 33), key(20, R1, 33), key(21, K1, 65), key(21, R1, 65),
                                                key(22, RSA, 140)]
    must, sigs, status, allowed = [], [], [], set()
    for _ in range(ntx):
        must.append([random_tree(rng, pool, 3) for _ in range(rng.choice((0, 1, 1, 1, 2, 3)))])
        sigs.append(rng.sample(pool, rng.randint(1, 6)))
        status.append(OK if rng.random() < 0.85 else rng.choice((1, 2, 3, 4, 5, 6, 9)))
        if rng.random() < 0.04:
            sigs[-1], status[-1] = [], NO_SIGS
        if must[-1] and rng.random() < 0.15:
            allowed.add(rng.choice(must[-1]))
    return must, sigs, status, allowed


def test_random_transactions_against_the_python_rule():
    must, sigs, status, allowed = random_batch(20261019, 4000)
    got, _ = check_against_rule(must, sigs, status, allowed)
    # the generator reaches every req_status value and all three outcomes of an evaluated transaction
    assert {r for g in got for r in g[1]} == {FULFILLED, MISSING, ALLOWED, NOT_EVALUATED, MALFORMED}
    evaluated = {g[0] for g, s in zip(got, status) if s == OK}
    assert evaluated == {OK, MISSING_TX, BAD_COVER}
    assert any(g[0] == OK and ALLOWED in g[1] for g in got)  # an allowed key alone does not fail its transaction


# ---- MALFORMED, class by class -----------------------------------------------------
def raw(tx_reqs, keys, sig_keys, status=None):
    """Token streams given directly: tx_reqs[t] = [tokens] with tokens = [(nchild, weight, threshold, key)]."""
    cov = C.CoverArrays([[(toks, False) for toks in per] for per in tx_reqs], keys)
    st, req, fm = C.cover_eval_host(cov, [OK] * len(tx_reqs) if status is None else status, sig_keys)
    return [int(x) for x in st], [int(x) for x in req], [int(x) for x in fm]


LEAF0, LEAF1 = (0, 1, 0, 0), (0, 1, 0, 1)


@pytest.mark.parametrize("name,tokens,want", [
    ("empty token range", [], MALFORMED),
    ("two values left", [LEAF0, LEAF1], MALFORMED),
    ("three values, one node over two", [LEAF0, LEAF0, LEAF1, (2, 1, 1, 0)], MALFORMED),
    ("a lone node", [(2, 1, 1, 0)], MALFORMED),
    ("a node first", [(2, 1, 1, 0), LEAF0, LEAF1], MALFORMED),
    ("nchild 1", [LEAF0, (1, 1, 1, 0)], MALFORMED),
    ("more children than values", [LEAF0, LEAF1, (3, 1, 1, 0)], MALFORMED),
    ("nchild 2^32 - 1", [LEAF0, LEAF1, (2**32 - 1, 1, 1, 0)], MALFORMED),
    ("threshold 0", [LEAF0, LEAF1, (2, 1, 0, 0)], MALFORMED),
    ("threshold = total", [LEAF0, LEAF1, (2, 1, 2, 0)], FULFILLED),
    ("threshold = total + 1", [LEAF0, LEAF1, (2, 1, 3, 0)], MALFORMED),
    ("threshold 2^31", [LEAF0, LEAF1, (2, 1, 2**31, 0)], MALFORMED),
    ("child weight 0", [(0, 0, 0, 0), LEAF1, (2, 1, 1, 0)], MALFORMED),
    ("child weight 2^31", [(0, 2**31, 0, 0), LEAF1, (2, 1, 1, 0)], MALFORMED),
    ("child weight 2^32 - 1", [(0, 2**32 - 1, 0, 0), LEAF1, (2, 1, 1, 0)], MALFORMED),
    ("inner node weight 0", [LEAF0, LEAF1, (2, 0, 1, 0), LEAF1, (2, 1, 1, 0)], MALFORMED),
    ("total weight 2^31 - 1", [(0, 2**31 - 2, 0, 0), LEAF1, (2, 1, 2**31 - 1, 0)], FULFILLED),
    ("total weight 2^31", [(0, 2**31 - 1, 0, 0), LEAF1, (2, 1, 1, 0)], MALFORMED),
    ("total weight 2^32 wraps to 0 in 32 bits", [(0, 2**31 - 1, 0, 0), (0, 2**31 - 1, 0, 1), (0, 2, 0, 0),
                                                 (3, 1, 1, 0)], MALFORMED),
    ("leaf key = nckey", [(0, 1, 0, 3)], MALFORMED),
    ("leaf key 2^32 - 1 inside a tree", [LEAF0, (0, 1, 0, 2**32 - 1), (2, 1, 1, 0)], MALFORMED),
    ("the root's weight is ignored", [LEAF0, LEAF1, (2, 0, 1, 0)], FULFILLED),
    ("a plain key's weight is ignored", [(0, 0, 0, 1)], FULFILLED),
])
def test_malformed_classes(name, tokens, want):
    keys = [ALICE, BOB, CHARLIE]
    st, req, fm = raw([[tokens]], keys, [[ALICE, BOB]])
    assert req == [want], name
    assert st == [BAD_COVER if want == MALFORMED else OK] and fm == [0 if want == MALFORMED else -1], name
    # a malformed entry does not disturb its neighbours, in the same transaction or the next
    st, req, fm = raw([[[LEAF0], tokens, [(0, 1, 0, 2)]], [[LEAF0, LEAF1, (2, 1, 2, 0)]]], keys,
                      [[ALICE, BOB], [ALICE, BOB]])
    assert req == [FULFILLED, want, MISSING, FULFILLED], name
    assert st == [BAD_COVER if want == MALFORMED else MISSING_TX, OK], name
    assert fm == [1 if want == MALFORMED else 2, -1], name


def test_constraint_cases_of_composite_key_tests():
    """CompositeKeyTests.kt:173-201 through flatten(): what the Kotlin builder refuses arrives as MALFORMED."""
    bad = [CK(1, ((ALICE, 0), (BOB, 1))), CK(0, ((ALICE, 1), (BOB, 1))), CK(5, ((ALICE, 2), (BOB, 2))),
           CK(2, ((ALICE, 3),)), CK(1, ((ALICE, INT_MAX), (BOB, INT_MAX))),
           node(ALICE, CK(0, ((ALICE, 1), (BOB, 1))))]
    got, _ = check_against_rule([[k] for k in bad], [[ALICE, BOB]] * len(bad))
    assert [g[0] for g in got] == [BAD_COVER] * len(bad)


# ---- key equality -------------------------------------------------------------------
def test_same_bytes_under_another_scheme_are_another_key():
    k1, r1 = key(7, K1, 33), key(7, R1, 33)
    k1u, r1u = key(8, K1, 65), key(8, R1, 65)
    must = [[k1], [k1], [r1u], [node(k1, r1)], [node(k1, r1)], [node(k1u, r1u, threshold=1)]]
    sigs = [[k1], [r1], [k1u], [k1, r1], [k1, k1], [r1u]]
    got, cov = check_against_rule(must, sigs)
    assert [g[0] for g in got] == [OK, MISSING_TX, MISSING_TX, OK, MISSING_TX, OK]
    assert cov.nckey == 4  # one table entry per (scheme, bytes)
    # a prefix or an extension of the bytes is another key too
    got, _ = check_against_rule([[key(9, ED, 32)]] * 3, [[key(9, ED, 31)], [key(9, ED, 33)], [key(9, ED, 32)]])
    assert [g[0] for g in got] == [MISSING_TX, MISSING_TX, OK]


def test_shared_key_table_entries():
    """Any number of leaves, of any transaction, may name one table entry; only the
    transaction's own signatures fulfil it."""
    tree = node(ALICE, node(ALICE, BOB, threshold=1), threshold=2)
    must = [[ALICE, tree, ALICE], [ALICE], [tree, BOB]]
    got, cov = check_against_rule(must, [[ALICE], [BOB], [BOB]])
    assert cov.nckey == 2 and cov.ntok == 14
    assert got == [(OK, [FULFILLED] * 3, -1), (MISSING_TX, [MISSING], 0), (MISSING_TX, [MISSING, FULFILLED], 0)]


# ---- per-transaction order ----------------------------------------------------------
def test_precedence():
    bad = CK(0, ((ALICE, 1), (BOB, 1)))
    must = [[CHARLIE, bad, BOB]] * 4 + [[]] * 2
    sigs = [[ALICE]] * 3 + [[]] + [[ALICE], []]
    status = [OK, 1, _lib.TX_NO_LEAVES, NO_SIGS, OK, NO_SIGS]
    got, _ = check_against_rule(must, sigs, status)
    assert got[0] == (BAD_COVER, [MISSING, MALFORMED, MISSING], 1)          # BAD_COVER over SIGNATURES_MISSING
    assert got[1] == (1, [NOT_EVALUATED] * 3, -1)                           # a failed signature over both
    assert got[2] == (_lib.TX_NO_LEAVES, [NOT_EVALUATED] * 3, -1)
    assert got[3] == (NO_SIGS, [NOT_EVALUATED] * 3, -1)
    assert got[4] == (OK, [], -1) and got[5] == (NO_SIGS, [], -1)           # no required keys
    for st in (2, 3, 4, 5, _lib.TX_BAD_COMPONENT):
        assert run([[CHARLIE]], [[ALICE]], [st])[0] == [(st, [NOT_EVALUATED], -1)]


def test_allowed_to_be_missing():
    tree = node(ALICE, BOB)
    must = [[ALICE, CHARLIE, tree], [CHARLIE], [CHARLIE, BOB], [tree, tree]]
    sigs = [[ALICE]] * 4
    got, cov = check_against_rule(must, sigs, allowed=[CHARLIE])
    assert got == [(MISSING_TX, [FULFILLED, ALLOWED, MISSING], 2), (OK, [ALLOWED], -1),
                   (MISSING_TX, [ALLOWED, MISSING], 1), (MISSING_TX, [MISSING, MISSING], 0)]
    got, _ = check_against_rule(must, sigs, allowed=[CHARLIE, tree, BOB])
    assert [g[0] for g in got] == [OK] * 4
    # the flag does not excuse a malformed key, and NULL flags mean none
    bad = CK(0, ((ALICE, 1), (BOB, 1)))
    assert run([[bad]], [[ALICE]], allowed=[bad])[0] == [(BAD_COVER, [MALFORMED], 0)]
    cov = C.flatten([[CHARLIE]], None)
    cov.req_flags = np.zeros(0, np.uint8)
    assert int(C.cover_eval_host(cov, [OK], [[ALICE]])[0][0]) == MISSING_TX


# ---- the CSR check ------------------------------------------------------------------
def test_bad_offsets_are_invalid_arg():
    def fresh():
        return C.flatten([[ALICE, node(ALICE, BOB)], [BOB]], None)

    sigs = [[ALICE], [BOB]]
    assert int(C.cover_eval_host(fresh(), [OK, OK], sigs)[0][0]) == MISSING_TX
    for field, idx, val in [("tx_req_off", 2, 4), ("tx_req_off", 1, 4), ("tx_req_off", 0, 2**63),
                            ("req_tok_off", 3, 6), ("req_tok_off", 1, 5), ("req_tok_off", 2, 2**64 - 1),
                            ("ckey_off", 2, 65), ("ckey_off", 1, 70), ("ckey_off", 0, 33)]:
        cov = fresh()
        getattr(cov, field)[idx] = val
        with pytest.raises(_lib.EngineError) as e:
            C.cover_eval_host(cov, [OK, OK], sigs)
        assert e.value.code == -1, (field, idx)
    for field, val in [("nreq", 2), ("ntok", 4), ("ckey_bytes", 63)]:  # a declared count below what the offsets span
        cov = fresh()
        c = cov.struct()
        setattr(c, field, val)
        st = np.zeros(2, np.uint8)
        so, sch, kb, ko = C.sig_key_arrays(sigs)
        rc = _lib.lib().cordahip_cover_eval_host(ctypes.byref(c), 2, st.ctypes.data, so.ctypes.data, sch.ctypes.data,
                                                 kb.ctypes.data, ko.ctypes.data, 2, kb.size)
        assert rc == -1, field
    # the signature level is checked the same way
    cov = fresh()
    c = cov.struct()
    so, sch, kb, ko = C.sig_key_arrays(sigs)
    for arr, idx, val in [(so, 2, 3), (so, 1, 9), (ko, 2, 65), (ko, 0, 40)]:
        a2 = [x.copy() for x in (so, ko)]
        (a2[0] if arr is so else a2[1])[idx] = val
        rc = _lib.lib().cordahip_cover_eval_host(ctypes.byref(c), 2, np.zeros(2, np.uint8).ctypes.data,
                                                 a2[0].ctypes.data, sch.ctypes.data, kb.ctypes.data, a2[1].ctypes.data,
                                                 2, kb.size)
        assert rc == -1
    assert _lib.lib().cordahip_cover_eval_host(None, 2, None, None, None, None, None, 0, 0) == -1
    assert _lib.lib().cordahip_cover_eval_host(ctypes.byref(c), 0, None, None, None, None, None, 0, 0) == 0


# ---- resolve.verify_signatures_batch_covered ------------------------------------------
class CoveredOracleEngine:
    """signed_tx_verify_covered with the C-ABI's contract on the CPU: the oracle engine of
    test_resolve.py for the signature half, cordahip_cover_eval_host for coverage."""

    def __init__(self, oracle):
        import test_resolve as TR
        self.inner = TR.OracleEngine(oracle)

    def signed_tx_verify(self, txs, sigs):
        return self.inner.signed_tx_verify(txs, sigs)

    def signed_tx_verify_covered(self, txs, sigs, cover):
        ids, tx_st, first_bad, sig_st = self.inner.signed_tx_verify(txs, sigs)
        st, req, fm = C.cover_eval_host(cover, tx_st, sigs)
        return ids, st, first_bad, sig_st, req, fm


def same_outcomes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.id == y.id and x.first_bad_sig == y.first_bad_sig
        assert type(x.error) is type(y.error)
        if isinstance(x.error, R.SignaturesMissingException):
            assert x.error.missing == y.error.missing and x.error.descriptions == y.error.descriptions
            assert x.error.id == y.error.id and str(x.error) == str(y.error)
        elif x.error is not None:
            assert str(x.error) == str(y.error)


def test_verify_signatures_batch_covered_equals_the_python_path(oracle):
    import test_resolve as TR
    pubs = [TR._ed_pub(oracle, s) for s in TR.SEEDS]
    a, b, c, d = pubs
    two_of_three = CK(2, ((a, 1), (b, 1), (c, 1)))
    ab_or_c = CK(1, ((CK(2, ((a, 1), (b, 1))), 1), (c, 1)))
    stxs = [
        TR._issue(oracle, b"t0", signers=(0,))[0],
        TR._issue(oracle, b"t1", signers=(0,), must=[a, b])[0],
        TR._issue(oracle, b"t2", signers=(0, 1), must=[two_of_three, ab_or_c])[0],
        TR._issue(oracle, b"t3", signers=(2,), must=[two_of_three, ab_or_c, d, two_of_three, d])[0],
        TR._issue(oracle, b"t4", signers=(), must=[a])[0],
        TR._issue(oracle, b"t5", signers=(0,), must=[b, a, b, c])[0],
        TR._issue(oracle, b"t6", signers=(1,), must=[d])[0],
        TR._issue(oracle, b"t7", signers=(3,), must=[])[0],
    ]
    stxs[3].commands = [("Move", [two_of_three]), ("Issue", [d, a]), ("Exit", [ab_or_c])]
    stxs[3].notary = d
    stxs[5].commands = [("Move", [b]), ("Issue", [a])]
    stxs[5].notary = c
    stxs.append(R.SignedTx([], [(ED, a, bytes(64))], [a]))                           # no leaves
    bad = TR._issue(oracle, b"t9", signers=(0, 1), must=[c])[0]
    bad.sigs[1] = (ED, b, bytes(64))                                                  # a failing signature
    stxs.append(bad)
    eng = CoveredOracleEngine(oracle)
    for allowed in ((), (d,), (b, c, d), (two_of_three,)):
        want = R.verify_signatures_batch(eng, stxs, allowed)
        got = R.verify_signatures_batch_covered(eng, stxs, allowed)
        same_outcomes(got, want)
    kinds = [type(o.error) for o in R.verify_signatures_batch_covered(eng, stxs)]
    assert R.SignaturesMissingException in kinds and type(None) in kinds and R.MerkleTreeException in kinds
    assert R.IllegalArgumentException in kinds and R.SignatureException in kinds
    # what checkValidity rejects is an IllegalArgumentException, ahead of any missing signer
    broken = TR._issue(oracle, b"t10", signers=(0,), must=[b, CK(0, ((a, 1), (b, 1)))])[0]
    o = R.verify_signatures_batch_covered(eng, [broken])[0]
    assert isinstance(o.error, R.IllegalArgumentException) and o.id is not None
    assert R.verify_signatures_batch_covered(eng, []) == []


# ---- struct layouts --------------------------------------------------------------------
def test_cover_struct_layouts_match_header(tmp_path):
    """cordahip_cover and cordahip_cover_tok as ctypes (and numpy) lay them out == gcc's
    layout of include/cordahip.h, with the method of test_abi.test_struct_layouts_match_header."""
    if shutil.which("gcc") is None:
        pytest.skip("gcc absent")
    structs = {"cordahip_cover": _lib.Cover, "cordahip_cover_tok": _lib.CoverTok}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cordahip.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    for name in ("CORDAHIP_TX_SIGNATURES_MISSING", "CORDAHIP_TX_BAD_COVER", "CORDAHIP_REQ_FULFILLED",
                 "CORDAHIP_REQ_MISSING", "CORDAHIP_REQ_MISSING_ALLOWED", "CORDAHIP_REQ_NOT_EVALUATED",
                 "CORDAHIP_REQ_MALFORMED"):
        lines.append('printf("%s %%d\\n", %s);' % (name, name))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    assert ctypes.sizeof(_lib.CoverTok) == 16 == _lib.COVER_TOK_DTYPE.itemsize
    assert [_lib.COVER_TOK_DTYPE.fields[f[0]][1] for f in _lib.CoverTok._fields_] == [0, 4, 8, 12]
    assert (int(got["CORDAHIP_TX_SIGNATURES_MISSING"]), int(got["CORDAHIP_TX_BAD_COVER"])) == \
        (_lib.TX_SIGNATURES_MISSING, _lib.TX_BAD_COVER) == (10, 11)
    assert [int(got["CORDAHIP_REQ_" + n]) for n in ("FULFILLED", "MISSING", "MISSING_ALLOWED", "NOT_EVALUATED",
                                                    "MALFORMED")] == \
        [_lib.REQ_FULFILLED, _lib.REQ_MISSING, _lib.REQ_MISSING_ALLOWED, _lib.REQ_NOT_EVALUATED,
         _lib.REQ_MALFORMED] == [0, 1, 2, 3, 4]
