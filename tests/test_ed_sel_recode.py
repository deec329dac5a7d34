"""The Ed25519 ladder's selector stream (corda_amd/csrc/ed25519_sel.hpp) on the
host under AddressSanitizer + UBSan: tools/ed_sel_check.cpp compares what
sel_recode writes -- one 5-bit selector per joint window, the window count, the
16 fixed-base digits as magnitude and sign -- with joint_booth2 / joint_select /
booth_digit<16> window by window, and rebuilds |c0|, c1 and e from the stream
alone. Scalars: 0, 1, 2^127, 2^128 - 1, 2^128, 2^129 - 1, 2^158, 2^159 - 1, 2^159
(the first bit that needs the high windows), 2^255, 2^256 - 1 and the 0xAA.. /
0x55.. patterns over 128 and 256 bits in every pairing, e up to 2^253 - 1 and
L - 1, both signs of c0, and 10^5 seeded random triples (|c0|, c1 of 120-134 bits,
every seventh / eleventh of any length up to 256; e with its top bits set in
every fifth)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_selector_stream_matches_window_recoding_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ed_sel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ed_sel_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "100000", "20261020"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    # 15 x 15 pairs of scalars x 9 values of e x 2 signs of c0
    assert st["fixed_cases"] == 15 * 15 * 9 * 2, st
    assert st["random_cases"] == 100000, st
