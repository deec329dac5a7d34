"""OpenSSL accepts the RSA signer's signatures: the host reference of the kernel's schedule
(corda_amd/csrc/rsa_sign.hpp through tools/rsa_sign_check.cpp) signs under every accepted golden
key, and the local libcrypto -- an independent RSASSA-PSS verifier, which also enforces RFC 8017
9.1.2 step 6 on the bits above emBits -- takes each signature and refuses it over another
message. Skipped where libcrypto 3 does not load."""
import json
import os
import shutil
import subprocess

import pytest

import rsa_sign_model as model

try:
    import openssl_rsa_pss as ossl
    ossl.lib()
except (OSError, AttributeError) as exc:  # no libcrypto 3 on this machine
    pytest.skip("OpenSSL libcrypto cannot be loaded: %s" % exc, allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_openssl_accepts_reference_signatures(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    exe = str(tmp_path / "rsa_sign_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "rsa_sign_check.cpp")])
    keys = model.accepted_keys()
    cases = [(k, model.message(40 + i, n), model.salt(40 + 3 * i + j))
             for i, k in enumerate(keys) for j, n in enumerate((1, 32, 200))]
    lines = ["sign %s %d %s %s" % (" ".join("%x" % v for v in k.crt()), k.e, m.hex(), s.hex()) for k, m, s in cases]
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [json.loads(l) for l in p.stdout.strip().splitlines()]
    assert len(out) == len(cases)
    taken = 0
    for (k, m, s), r in zip(cases, out):
        sig = bytes.fromhex(r["sig"])
        assert r["ok"] is True and sig == k.sign(m, s)
        got = ossl.verify(k.der(), sig, m)
        assert got is not False, (k.name, len(m))  # None: OpenSSL does not take the key itself
        if got:
            taken += 1
            assert ossl.verify(k.der(), sig, m + b"?") is False
    assert taken >= 3 * 8  # the OpenSSL-made keys and the 65537 ones at the least
