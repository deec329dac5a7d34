"""The ECDSA signer's model (tests/ecdsa_sign_model.py) pinned on RFC 6979's own vectors
(tests/golden/rfc6979_vectors.json: A.2.5 P-256 / SHA-256 "sample" and "test", and the
widely published secp256k1 vector, whose s there is the low-half form n - s of ours),
checked by independent verifiers (the C oracle's oracle_ecdsa_verify, the local
openssl where present), and the golden file tests/golden/ecdsa_sign_vectors.json
against the model: every 16th case re-derived, every property the kernel's paths need
present for both curves. Also the branch-free mixed addition's model: the comb run from
the top digit with a chord-only addition that raises on a doubling or an inverse."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import ecdsa_sign_model as M
import make_ecdsa_sign_vectors as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def rfc():
    return json.load(open(os.path.join(GOLDEN, "rfc6979_vectors.json")))["vectors"]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "ecdsa_sign_vectors.json")))


def test_rfc6979_vectors(rfc):
    assert len(rfc) == 3
    for v in rfc:
        c, d, msg = M.CURVES[v["scheme"]], int(v["x"], 16), v["msg"].encode()
        k, tries = M.nonce(d, hashlib.sha256(msg).digest(), c.n)
        assert (k, tries) == (int(v["k"], 16), 1), v["msg"]
        r, s, k2 = M.sign_rs(c, d, msg)
        assert (r, s, k2) == (int(v["r"], 16), int(v["s"], 16), k), v["msg"]
        assert M.sign(c, d, msg) == M.der_sig(r, s) == M.sign_like_kernel(c, d, msg)
        assert M.verify(c, M.public_key(c, d), msg, r, s)
    # the secp256k1 vector is usually published with the low-half s: ours is n - that
    assert M.K1.n - int(rfc[2]["s"], 16) == 0x2442CE9D2B916064108014783E923EC36B49743E2FFA1C4496F01A512AAFD9E5


def _model_signatures(rfc, golden):
    """(scheme, pub, msg, der) of the RFC vectors and every golden case"""
    out = []
    for v in rfc:
        c, d, msg = M.CURVES[v["scheme"]], int(v["x"], 16), v["msg"].encode()
        out.append((c.scheme, M.public_key(c, d), msg, M.der_sig(int(v["r"], 16), int(v["s"], 16))))
    for cs in golden["cases"]:
        key = golden["keys"][cs["key"]]
        out.append((key["scheme"], bytes.fromhex(key["pub"]), bytes.fromhex(cs["msg"]), bytes.fromhex(cs["sig"])))
    return out


def test_model_signatures_verify_under_the_c_oracle(oracle, rfc, golden):
    sigs = _model_signatures(rfc, golden)
    for scheme, pub, msg, der in sigs:
        assert oracle.oracle_ecdsa_verify(scheme, pub, len(pub), der, len(der), msg, len(msg)) == 0
        bad = bytes([msg[0] ^ 1]) + msg[1:]
        assert oracle.oracle_ecdsa_verify(scheme, pub, len(pub), der, len(der), bad, len(bad)) != 0


_SPKI = {2: bytes.fromhex("3056301006072a8648ce3d020106052b8104000a034200"),
         3: bytes.fromhex("3059301306072a8648ce3d020106082a8648ce3d030107034200")}


@pytest.mark.skipif(shutil.which("openssl") is None, reason="openssl absent")
def test_model_signatures_verify_under_openssl(tmp_path, rfc, golden):
    sigs = _model_signatures(rfc, golden)
    picked = sigs[:3] + sigs[3::8]  # the RFC vectors and every 8th golden case, both curves
    assert {s[0] for s in picked} == {2, 3}
    for i, (scheme, pub, msg, der) in enumerate(picked):
        kf, sf, mf = tmp_path / ("k%d.der" % i), tmp_path / ("s%d.bin" % i), tmp_path / ("m%d.bin" % i)
        kf.write_bytes(_SPKI[scheme] + pub)
        sf.write_bytes(der)
        mf.write_bytes(msg)
        p = subprocess.run(["openssl", "dgst", "-sha256", "-verify", str(kf), "-keyform", "DER", "-signature", str(sf),
                            str(mf)], capture_output=True, text=True)
        if i == 0 and p.returncode != 0 and "Verif" not in p.stdout:
            pytest.skip("this openssl does not read the key: " + p.stderr[-200:])
        assert p.returncode == 0 and "Verified OK" in p.stdout, (i, scheme, p.stdout, p.stderr)


def test_golden_file_against_the_model(golden):
    keys, cases = golden["keys"], golden["cases"]
    assert len(cases) <= 400 and tuple(golden["lengths"]) == G.LENGTHS
    for c in (M.K1, M.R1):
        mine = [k for k in keys if k["scheme"] == c.scheme]
        ds = [int(k["d"], 16) for k in mine]
        assert 1 in ds and c.n - 1 in ds and any(len(k["d"]) == 64 and k["d"].startswith("0000") and int(k["d"], 16) > 1
                                                 for k in mine)
        for k in mine:
            assert 0 < int(k["d"], 16) < c.n
        have, lens = set(), set()
        for cs in cases:
            if keys[cs["key"]]["scheme"] != c.scheme:
                continue
            have.update(cs["props"])
            lens.add(len(cs["msg"]) // 2)
            sig = bytes.fromhex(cs["sig"])
            assert len(sig) <= 72 and sig[0] == 0x30 and sig[1] == len(sig) - 2
        assert not [p for p in G.REQUIRED if p not in have], (c.name, have)
        assert lens >= set(G.LENGTHS)
    # the public keys, and every 16th case, from the model (the properties of every case from its numbers)
    for k in keys[::3]:
        assert M.public_key(M.CURVES[k["scheme"]], int(k["d"], 16)).hex() == k["pub"]
    for i, cs in enumerate(cases):
        key = keys[cs["key"]]
        c, d, msg = M.CURVES[key["scheme"]], int(key["d"], 16), bytes.fromhex(cs["msg"])
        if i % 16 == 0:
            r, s, k = M.sign_rs(c, d, msg)
            assert M.der_sig(r, s).hex() == cs["sig"] and "%064x" % k == cs["k"], i
            assert G.properties(c, k, r, s, M.der_sig(r, s)) == cs["props"], i


def test_branch_free_addition_model(golden):
    """The selection rule of jmadd_ct over every golden nonce: from the top digit, the general (chord)
    addition never meets the accumulator's own point or its inverse, the accumulator leaves infinity at
    the first non-zero digit, and the result is [k']G."""
    keys, cases = golden["keys"], golden["cases"]
    seen = {2: set(), 3: set()}
    for i, cs in enumerate(cases):
        c = M.CURVES[keys[cs["key"]]["scheme"]]
        k = int(cs["k"], 16)
        kp, flip = M.split_min(k, c.n)
        assert kp < 1 << 255 and kp == min(k, c.n - k)
        digits, carry = M.recode(kp)
        assert carry == 0 and all(-7 <= d <= 8 for d in digits) and sum(d << (4 * j) for j, d in enumerate(digits)) == kp
        P, trace = M.comb_mult(c, kp)  # raises ExceptionalAddition on a doubling or an inverse
        top = max(j for j in range(64) if digits[j])
        assert all(trace[j] == "keep" for j in range(top + 1, 64)) and trace[top] == "lift"
        assert all(trace[j] == ("sum" if digits[j] else "keep") for j in range(top))
        seen[c.scheme].update(trace.values())
        if "top3zero" in cs["props"]:
            assert top <= 60
            seen[c.scheme].add("late")
        if i % 8 == 0 or "top3zero" in cs["props"]:
            Q = M.mul(c, k, c.G)
            assert P[0] == Q[0] and P == (M.neg(c, Q) if flip else Q)
    for s in (2, 3):
        assert seen[s] == {"keep", "lift", "sum", "late"}
    # the boundary scalars
    for c in (M.K1, M.R1):
        for kp in (1, (c.n - 1) // 2, 8 << 252, (1 << 255) - 1, 0x8888 << 236):
            P, _ = M.comb_mult(c, kp)
            assert P == M.mul(c, kp, c.G)
    with pytest.raises(M.ExceptionalAddition):
        M.general_add(M.R1, M.R1.G, M.neg(M.R1, M.R1.G))
