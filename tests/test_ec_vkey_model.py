"""CPU model of the keyed ECDSA verifier (tests/ec_vkey_model.py: integer window tables of the key
and of the base point, ecdsa_vkey.hpp's digit rule and order of additions, no scalar multiplication)
against the oracle: the model's status equals oracle/bc_ecdsa.verify_status on every lane of
tests/golden/ecdsa_vectors.json whose key registers (738 of 832: the other 94 belong to keys that are
not points, whose every vector is BAD_KEY) and on all 66 lanes of tests/golden/cert_vectors.json,
under doVerify rules, and under isValid rules where the two differ (empty signature or message).
The base-point half is a table sum too: a wrong G table cannot hide behind the oracle's
multiplication."""
import collections
import json
import os

import bc_ecdsa as bc
import ec_vkey_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vectors(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)["vectors"]


def _check(vectors):
    """Registers every key once (a table per distinct (scheme, key bytes)); returns
    (lanes run, lanes left out, events summed over the lanes run)."""
    tables = {}
    by_key = collections.defaultdict(list)
    for v in vectors:
        by_key[(v["scheme"], v["pub"])].append(v)
    ran = skipped = 0
    total = collections.Counter()
    for (scheme, pub), vs in by_key.items():
        q = bc.decode_point(bc.CURVES[scheme], bytes.fromhex(pub))
        if q is None:  # the add answers BAD_KEY: nothing to verify against
            assert all(v["status"] == bc.BAD_KEY for v in vs)
            skipped += len(vs)
            continue
        tab = tables[(scheme, pub)] = model.point_table(bc.CURVES[scheme], q)
        for v in vs:
            sig, msg = bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])
            # isValid differs from doVerify in the emptiness checks alone: the oracle is asked
            # again only where they bite
            for is_valid in ((False, True) if not sig or not msg else (False,)):
                got, ev = model.model_status(scheme, tab, sig, msg, is_valid)
                want = bc.verify_status(scheme, bytes.fromhex(pub), sig, msg, is_valid)
                assert got == want, (v["cat"], v.get("note", ""), is_valid, got, want)
                if not is_valid:
                    assert got == v["status"], (v["cat"], got, v["status"])
                    if ev:
                        total.update(ev)
            ran += 1
    return ran, skipped, total


def test_base_table_is_a_table_of_g():
    """Entries of the G tables against the oracle's multiplication, at both ends of both ranges."""
    for scheme, c in bc.CURVES.items():
        tab = model.g_table(scheme)
        for j, d in ((0, 1), (0, 128), (1, 1), (17, 77), (31, 1), (31, 128)):
            assert tab[j][d] == bc._mul(c, d << (8 * j), c.G), (scheme, j, d)


def test_model_equals_oracle_on_golden_vectors():
    ran, skipped, ev = _check(_vectors("ecdsa_vectors.json"))
    assert (ran, skipped) == (738, 94)
    assert ev["zero"] > 0  # skipped additions occur


def test_model_equals_oracle_on_reference_certificates():
    vs = _vectors("cert_vectors.json")
    assert len(vs) == 66
    ran, skipped, _ = _check(vs)
    # a certificate lane whose key is not a point keeps its recorded BAD_KEY (checked in _check)
    assert ran + skipped == 66 and ran > 0


def test_scalar_trace_matches_point_trace():
    """The scalar-domain search the GPU tests use sees the same events as the point model."""
    import hashlib
    for scheme, c in bc.CURVES.items():
        for dq in (1, c.n - 1, 0xC0FFEE):
            q = bc._mul(c, dq, c.G)
            tab = model.point_table(c, q)
            for i in range(12):
                h = hashlib.sha256(b"trace-%d-%d" % (scheme, i)).digest()
                u1 = int.from_bytes(h, "big") % c.n
                u2 = int.from_bytes(hashlib.sha256(h).digest(), "big") % c.n
                if i == 0:
                    u1, u2 = 5, 5  # Q = G: the key's entry meets the accumulator it equals
                pt, ev = model.trace(scheme, tab, u1, u2)
                acc, sev = model.scalar_trace(c.n, dq, u1, u2)
                assert ev == sev, (scheme, dq, i, ev, sev)
                assert pt == (bc._mul(c, acc, c.G) if acc else None)
            if dq == 1:
                assert model.scalar_trace(c.n, 1, 5, 5)[1]["dbl"] == 1
            if dq == c.n - 1:
                assert model.scalar_trace(c.n, dq, 5, 5)[1]["inf"] == 1
