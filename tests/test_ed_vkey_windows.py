"""The keyed Ed25519 verifier's window geometry (corda_amd/csrc/ed25519_vkey.hpp) on the
host under AddressSanitizer + UBSan: tools/ed_vkey_check.cpp checks, for 0, 1, L - 1,
2^252, the full carry chains (bytes 0..30 all 0x7f, 0x80 or 0x81 under a top byte of 0 and
of 0x10), a single byte 0x80 and 0x81 at every position, and 10^5 seeded scalars reduced
below L with the kernel's own sc_reduce512 (sc25519.hpp), that the 32 signed digits satisfy
|d_j| <= 128 and sum_j d_j 256^j == h with no carry out of digit 31, that the kernel's
biased-word form and the byte-by-byte form yield the same digits, that every entry offset
stays inside the key's table, and that the key-id encoding round-trips slot and counter."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_vkey_windows_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ed_vkey_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ed_vkey_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "100000", "20261019"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True
    # 4 fixed + 3 x 2 chains + 2 x 32 single bytes + the random ones
    assert st["singles"] == 64 and st["randoms"] == 100000 and st["scalars"] == 4 + 6 + 64 + 100000, st
    # both ends of the digit range occur: 128 (a byte 0x80 with no carry in) and -127 (a byte 0x81);
    # zero digits (the identity entry) occur too
    assert st["max_abs"] == 128 and st["most_positive"] == 128 and st["most_negative"] == 127, st
    assert st["zero_digits"] > 1000, st
