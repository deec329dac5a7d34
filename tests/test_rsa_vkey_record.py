"""The registered RSA keys' record and schedule on the CPU under AddressSanitizer + UBSan:
tools/rsa_vkey_check.cpp includes corda_amd/csrc/rsa_vkey.hpp (no HIP), builds the record of
every key of tests/golden/rsa_pss_vectors.json and of the adversarial moduli of the GPU tests
with e in {3, 17, 65537, 2^32 - 1}, and runs the kernel's schedule (modexp_keyed) against
rsa::modexp. Here the records are checked against Python integers: n' = -n^-1 mod 2^32,
K = 2^(32 W e) mod n, the bit length and the width class; declined and malformed keys give
parse_public_key's statuses and leave the record untouched."""
import json
import os
import random
import shutil
import subprocess

import pytest

import bc_rsa_pss as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPONENTS = (3, 17, 65537, (1 << 32) - 1)


def class_words(bits):
    return 64 if bits <= 2048 else 96 if bits <= 3072 else 128


def adversarial_moduli(rng, w):
    """the set of test_gpu_rsa.py::adversarial_moduli"""
    r = 1 << (32 * w)
    return [r - 1, (1 << (32 * w - 1)) + 1, (rng.getrandbits(32 * w - 97) << 96) | ((1 << 96) - 1) | (1 << (32 * w - 1)),
            rng.getrandbits(32 * w) | 1 | (1 << (32 * w - 1)), rng.getrandbits(32 * w - 700) | 1,
            rng.getrandbits(32 * w - 31) | 1]


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    exe = str(tmp_path_factory.mktemp("rsa_vkey") / "rsa_vkey_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tools", "rsa_vkey_check.cpp")])

    def run(lines):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
        out = [json.loads(l) for l in p.stdout.strip().splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def check_record(r, n, e, w):
    assert r["status"] == 0
    assert r["e"] == e and r["bits"] == n.bit_length() and r["words"] == w == class_words(n.bit_length())
    assert int(r["n"], 16) == n  # zero above the class's words too
    assert r["np"] == -pow(n, -1, 2 ** 32) % 2 ** 32
    assert int(r["K"], 16) == pow(2, 32 * w * e, n)
    assert r["mismatch"] == 0  # in = 0, 1, n - 1 and four random values: modexp_keyed == rsa::modexp
    assert r["refused"] == 2  # in = n and in > n: false, a zero row
    assert int(r["out"], 16) == pow(int(r["in"], 16), e, n)


def test_golden_keys(tool):
    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        keys = json.load(f)["keys"]
    ders = [bytes.fromhex(k["der"]) for k in keys] + [b""]
    out = tool(["key " + (d.hex() or "-") for d in ders])
    good = bad = 0
    for d, r in zip(ders, out):
        want = bc.decode_key(d)
        if isinstance(want, int):
            assert r == {"status": want, "untouched": True}, (d.hex()[:40], r)
            bad += 1
        else:
            n, e = want
            check_record(r, n, e, class_words(n.bit_length()))
            good += 1
    assert good == 11 and bad == 10 + 1
    assert {r["status"] for r in out} == {bc.OK, bc.BAD_KEY, bc.UNSUPPORTED}


@pytest.mark.parametrize("w", (64, 96, 128))
def test_adversarial_moduli(tool, w):
    rng = random.Random(0x18 + w)
    mods = adversarial_moduli(rng, w)
    if w == 64:
        mods.append(rng.getrandbits(1024) | 1 | (1 << 1023))  # a 1024-bit key in the 2048-bit class
    cases = [(n, e) for n in mods for e in EXPONENTS]
    out = tool(["mod %d %x %d" % (w, n, e) for n, e in cases])
    for (n, e), r in zip(cases, out):
        check_record(r, n, e, w)
