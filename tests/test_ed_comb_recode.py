"""The Ed25519 signer's comb recoding (corda_amd/csrc/ed25519_comb.hpp) on the host
under AddressSanitizer + UBSan: tools/ed_comb_check.cpp checks, for 0, 1, L - 1,
2^252, the full carry chains (nibbles 0..62 all 7, 8, 9 or f under a top nibble of 0
and of 1 -- a scalar below 2^253 has no larger one -- and all 64 nibbles 7), a single
nibble 8 and 9 at every position, and 10^5 seeded random scalars below L, that the 64
signed digits satisfy |d_j| <= 8 and sum_j d_j 16^j == r with no carry out of digit
63, and that the shifting form the kernel runs yields the same digits."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_comb_recode_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ed_comb_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ed_comb_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "100000", "20261019"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True
    # 4 fixed + 4 x 2 chains + all-7 + 2 x 64 single nibbles + the random ones
    assert st["singles"] == 128 and st["randoms"] == 100000 and st["scalars"] == 4 + 8 + 1 + 128 + 100000, st
    # both ends of the digit range occur: 8 (a nibble 8 with no carry in) and -7 (a nibble 9)
    assert st["max_abs"] == 8 and st["most_positive"] == 8 and st["most_negative"] == 7, st
