"""The RSA signer's record and schedule on the CPU under AddressSanitizer + UBSan:
tools/rsa_sign_check.cpp includes corda_amd/csrc/rsa_sign.hpp (no HIP), builds the record of
every golden key that keeps p and q, and runs the kernel's schedule word-serially -- the
reduction of EM mod p and mod q, the fixed windows, the recombination and the fault check.
Here everything is checked against Python integers: every field of the record, raw private
operations, whole signatures against bc_rsa_pss.encode_em + sign_crt, and the status of every
key an add must turn down."""
import os
import random
import shutil
import subprocess
import json

import pytest

import bc_rsa_pss as bc
import rsa_sign_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    exe = str(tmp_path_factory.mktemp("rsa_sign") / "rsa_sign_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tools", "rsa_sign_check.cpp")])

    def run(lines):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        out = [json.loads(l) for l in p.stdout.strip().splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def hx(v):
    return "-" if v is None else "%x" % v


def key_args(comp, e):
    return " ".join(hx(v) for v in comp) + " %d" % e


@pytest.fixture(scope="module")
def keys():
    return model.accepted_keys()


def test_record_fields(tool, keys):
    assert len(keys) == 11
    out = tool(["key " + key_args(k.crt(), k.e) for k in keys])
    for k, r in zip(keys, out):
        w, wp = k.words, k.words // 2
        assert r["status"] == 0 and r["id"] == 0, k.name
        assert (r["e"], r["bits"], r["words"]) == (k.e, k.bits, w), k.name
        assert r["pbits"] == max(k.p.bit_length(), k.q.bit_length())
        for name, mod in (("np", k.n), ("npp", k.p), ("npq", k.q)):
            assert r[name] == -pow(mod, -1, 2 ** 32) % 2 ** 32, (k.name, name)
        for name, want in (("n", k.n), ("p", k.p), ("q", k.q), ("dp", k.dp), ("dq", k.dq), ("qinv", k.qinv),
                           ("K", pow(2, 32 * w * k.e, k.n)), ("qR", (k.q << (32 * w)) % k.n),
                           ("r2p", pow(2, 64 * wp, k.p)), ("r2q", pow(2, 64 * wp, k.q))):
            assert int(r[name], 16) == want, (k.name, name)  # zero above the class's words too
        assert r["consistent"] is True, k.name
    assert {k.words for k in keys} == {64, 96, 128}
    assert any(k.p > k.q for k in keys) and any(k.q > k.p for k in keys)


def test_raw_private_operation(tool, keys):
    rng = random.Random(0x19)
    cases = []
    for k in keys:
        ems = [0, 1, k.n - 1] + [rng.randrange(k.n) for _ in range(2)]
        ems += [k.p * rng.randrange(1, k.q), k.q * rng.randrange(1, k.p)]  # m1 = 0; m2 = 0
        ems += [k.p, k.q]
        # the low half at its largest, next to the top of the range (lo >= p and lo >= q)
        half = 1 << (16 * k.words)
        ems += [(k.n - 1) // half * half - 1, half - 1]
        cases += [(k, em) for em in ems if 0 <= em < k.n]  # a 1024-bit modulus is below one half word row
    out = tool(["raw %s %x" % (key_args(k.crt(), k.e), em) for k, em in cases])
    for (k, em), r in zip(cases, out):
        assert em < k.n
        assert r["ok"] is True, (k.name, hex(em)[:20])
        assert int(r["s"], 16) == bc.sign_crt(em, k.p, k.q, k.d) == pow(em, k.d, k.n), (k.name, hex(em)[:20])


def test_raw_refuses_what_the_fault_check_cannot_confirm(tool, keys):
    k = keys[0]
    out = tool(["raw %s %x" % (key_args(k.crt(), k.e), em) for em in (k.n, k.n + 1)])
    assert all(r["ok"] is False and int(r["s"], 16) == 0 for r in out)


def test_reduction_of_any_two_half_words(tool, keys):
    """EM of 2 Wp words whose halves are both above p and q: the products that fold the halves in
    take an operand that is merely below Rp"""
    rng = random.Random(0x1919)
    cases = []
    for k in keys:
        half = 1 << (16 * k.words)
        full = half * half
        top = max(k.p, k.q)
        ems = [full - 1, (top << (16 * k.words)) | top, ((half - 1) << (16 * k.words)) | (top + 1),
               (rng.randrange(top, half) << (16 * k.words)) | rng.randrange(top, half),
               k.p * (full // k.p), k.q * (full // k.q)]
        for em in ems[:4]:
            assert em >> (16 * k.words) >= top and em % half >= top
        cases += [(k, em) for em in ems]
    out = tool(["half %s %x" % (key_args(k.crt(), k.e), em) for k, em in cases])
    for (k, em), r in zip(cases, out):
        assert int(r["m1"], 16) == pow(em % k.p, k.dp, k.p), (k.name, hex(em)[:20])
        assert int(r["m2"], 16) == pow(em % k.q, k.dq, k.q), (k.name, hex(em)[:20])
    assert any(int(r["m1"], 16) == 0 for r in out) and any(int(r["m2"], 16) == 0 for r in out)


def test_signatures_equal_the_restatement(tool, keys):
    cases = [(k, model.message(i, n), model.salt(7 * i + j))
             for i, k in enumerate(keys) for j, n in enumerate(model.MSG_LENS)]
    out = tool(["sign %s %s %s" % (key_args(k.crt(), k.e), m.hex(), s.hex()) for k, m, s in cases])
    for (k, m, s), r in zip(cases, out):
        assert r["ok"] is True
        sig = bytes.fromhex(r["sig"])
        assert len(sig) == k.k and sig == k.sign(m, s), (k.name, len(m))
        assert bc.verify(k.der(), sig, m) == bc.OK


def test_rejected_keys(tool, keys):
    for k in (keys[0], keys[1], keys[2]):  # one per class
        cases = model.rejected_keys(k)
        out = tool(["key " + key_args(comp, e) for _, comp, e, _ in cases])
        for (what, _, _, want), r in zip(cases, out):
            if want == "consistency":  # the record builds; the consistency run is what turns it down
                assert r["status"] == 0 and r["consistent"] is False, (k.name, what)
            else:
                assert r == {"status": want, "zeroed": True}, (k.name, what, r)
    # leading zeros change nothing
    k = keys[0]
    pad = " ".join("0000" + hx(v) for v in k.crt()) + " %d" % k.e
    a, b = tool(["key " + pad, "key " + key_args(k.crt(), k.e)])
    assert a == b and a["consistent"] is True


def test_declined_golden_keys(tool):
    declined = [k for k in model.private_keys() if k.name in model.DECLINED]
    assert [k.name for k in declined] == list(model.DECLINED)
    for k in declined:
        assert bc.decode_key(k.der()) == bc.UNSUPPORTED  # the verifier's own rules
    # e = 2^32 + 1 does not fit the C call's uint32_t: the Python wrapper refuses it
    assert declined[2].e >= 1 << 32
    out = tool(["key " + key_args(k.crt(), k.e) for k in declined[:2]])
    assert out == [{"status": bc.UNSUPPORTED, "zeroed": True}] * 2


def test_restatement_verifies_for_every_private_golden_key():
    ks = model.private_keys()
    assert len(ks) == 14
    for i, k in enumerate(ks):
        m, s = model.message(i, 32), model.salt(i)
        assert bc.verify(k.der(), k.sign(m, s), m, decline=False) == bc.OK, k.name
        assert bc.verify(k.der(), k.sign(m, s), m + b"x", decline=False) == bc.BAD_SIG, k.name
