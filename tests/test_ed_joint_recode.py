"""The Ed25519 ladder's joint recoding (corda_amd/csrc/ed25519_joint.hpp) on the
host under AddressSanitizer + UBSan: tools/ed_joint_check.cpp checks that the
2-bit Booth digits of a scalar lie in [-2, 2] and sum to it over the ladder's
window count (0, 1, 2^127, 2^128 - 1, 2^131 and 10^5 seeded random scalars of
120-132 bits), and that for all 25 digit pairs and both signs of c0 the
(index, negate) pair of joint_select picks i P + j Q from a table filled in the
prep's order, with the group modelled as the integers mod L."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_joint_recode_and_index_map_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ed_joint_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ed_joint_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "100000", "20261019"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["scalars"] == 100000 + 5, st
    # 64 random (P, Q) x 2 signs of c0 x 25 digit pairs
    assert st["select_cases"] == 64 * 2 * 25, st
