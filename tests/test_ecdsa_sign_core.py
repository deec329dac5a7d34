"""The ECDSA signer's scalar side (corda_amd/csrc/ecdsa_sign_core.hpp) on the host under
AddressSanitizer + UBSan: tools/ecdsa_sign_check.cpp runs the header's RFC 6979 nonce
core against the Python model (tests/ecdsa_sign_model.py) -- the RFC's vectors, the
nonce of every golden case, and the retry path under the test modulus q = 2^255 + 95,
which rejects about half of all candidates (bound 64: each nonce and its number of
candidates equal the model's; bound 1: exhaustion exactly where the model needs a
second candidate) -- and checks the split k' = min(k, n - k) and the signed 4-bit
recoding: |d_j| <= 8, sum d_j 16^j == k', no carry out of digit 63, for k' = 1,
(n - 1) / 2, 2^255 - 1, the full carry chains and 10^5 seeded scalars below each n."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

import ecdsa_sign_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
Q_TEST = 2**255 + 95
RETRY_INPUTS = 200


def _line(q, bound, x, h1, k, tries):
    return "%x %d %x %s %x %d\n" % (q, bound, x, h1.hex(), k or 0, tries)


def _vectors():
    """(lines, retried under bound 64, exhausted under bound 1)"""
    lines = []
    for v in json.load(open(os.path.join(GOLDEN, "rfc6979_vectors.json")))["vectors"]:
        c = M.CURVES[v["scheme"]]
        lines.append(_line(c.n, M.MAX_TRIES, int(v["x"], 16), hashlib.sha256(v["msg"].encode()).digest(),
                           int(v["k"], 16), 1))
    g = json.load(open(os.path.join(GOLDEN, "ecdsa_sign_vectors.json")))
    for cs in g["cases"]:
        key = g["keys"][cs["key"]]
        c = M.CURVES[key["scheme"]]
        h1 = hashlib.sha256(bytes.fromhex(cs["msg"])).digest()
        k, tries = M.nonce(int(key["d"], 16), h1, c.n)
        assert k == int(cs["k"], 16)
        lines.append(_line(c.n, M.MAX_TRIES, int(key["d"], 16), h1, k, tries))
    retried = exhausted = 0
    for i in range(RETRY_INPUTS):
        x = int.from_bytes(hashlib.sha256(b"retry-x|%d" % i).digest(), "big") % (Q_TEST - 1) + 1
        h1 = hashlib.sha256(b"retry-m|%d" % i).digest()
        k, tries = M.nonce(x, h1, Q_TEST, 64)
        assert k is not None
        retried += tries > 1
        lines.append(_line(Q_TEST, 64, x, h1, k, tries))
        k1, t1 = M.nonce(x, h1, Q_TEST, 1)
        assert (k1 is None) == (tries > 1)
        exhausted += k1 is None
        lines.append(_line(Q_TEST, 1, x, h1, k1, t1))
    return lines, retried, exhausted


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_sign_core_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ecdsa_sign_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ecdsa_sign_check.cpp")])
    lines, retried, exhausted = _vectors()
    # the test modulus does reach the retry path: about half of the inputs
    assert RETRY_INPUTS // 4 < retried < 3 * RETRY_INPUTS // 4 and exhausted == retried, (retried, exhausted)
    vec = tmp_path / "nonces.txt"
    vec.write_text("".join(lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, str(vec), "100000", "20261020"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True
    assert st["nonces"] == len(lines) and st["retried"] == retried and st["exhausted"] == exhausted, st
    assert st["max_tries"] >= 3, st
    # per group order: 4 split cases, 2^255 - 1, 4 x 8 chains, the random ones
    assert st["scalars"] == 2 * (4 + 1 + 32 + 100000), st
    assert st["max_abs"] == 8 and st["most_positive"] == 8 and st["most_negative"] == 7, st
