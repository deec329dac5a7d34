"""The keyed ECDSA verifier's window geometry (corda_amd/csrc/ecdsa_vkey.hpp) and host packing
(pack_rows.hpp keyed_ec_pack_rows) on the host under AddressSanitizer + UBSan:
tools/ec_vkey_check.cpp checks, for both curves' n and the scalars 1, n - 1, 2^255 - 1, 2^255,
2^255 + 1, bytes all 0x80 / 0x81 / 0xff (reduced mod n) and 10^5 seeded scalars, that the sign
flag is (u >= 2^255), that the magnitude is below 2^255, that the biased sum has no carry out,
that the 32 signed digits satisfy |d_j| <= 128 and sum_j d_j 256^j equals the magnitude, that
the kernel's biased-word form and the byte-by-byte form agree and that every entry offset
stays inside the key's table; then the table, record and scratch offsets, the order of
additions, and keyed_ec_pack_rows on CSR batches in exact-size heap blocks (signatures of 0,
8, 72, 73 and 300 bytes, dense and ragged messages, both flags values)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_ec_vkey_windows_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ec_vkey_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ec_vkey_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "100000", "20261020"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True
    # per curve: 5 fixed + 3 equal-byte scalars + the random ones
    assert st["fixed"] == 16 and st["randoms"] == 200000 and st["scalars"] == 200016, st
    # about half of all scalars below n are >= 2^255 and take the negated form
    assert 90000 < st["negated"] < 110000, st
    # both ends of the digit range occur, and zero digits (skipped additions) too
    assert st["max_abs"] == 128 and st["most_positive"] == 128 and st["most_negative"] == 127, st
    assert st["zero_digits"] > 1000, st
    # 2 flags x (7 dense + 8 ragged lanes)
    assert st["pack_lanes"] == 30, st
