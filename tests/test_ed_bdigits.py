"""The fixed-base digits of the Ed25519 ladder's selector stream
(corda_amd/csrc/ed25519_sel.hpp) at each window width the header allows
(ED_B_BITS = 16, 18, 20), on the host under AddressSanitizer + UBSan:
tools/ed_bdigit_check.cpp, a program of its own, rebuilds e from the stream
alone (sum of d_t 2^(width t) over the header's low + high digit counts), bounds
every |d_t| by 2^(width - 1) and compares with booth_digit<width>. Values: 0, 1,
L - 1, 2^252, 2^253 - 1, the chunk patterns that make every digit exactly
-2^(width-1) or +2^(width-1) at even and odd positions, carries that ripple
through every digit and across the split between the digits over B and those
over B', and 10^5 seeded random e < L."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# width -> (digits over B, digits over B'): (lo + hi) width >= 254 and
# (lo - 1) width / 2 + 1 <= 64
SPLITS = {16: (8, 8), 18: (8, 7), 20: (7, 6)}


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
@pytest.mark.parametrize("bits", [16, 18, 20])
def test_fixed_base_digits_rebuild_e_asan_ubsan(tmp_path, bits):
    exe = str(tmp_path / ("ed_bdigit_check_%d" % bits))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-DED_B_BITS=%d" % bits,
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ed_bdigit_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "100000", "20261021"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    lo, hi = SPLITS[bits]
    assert (st["bits"], st["digits_lo"], st["digits_hi"]) == (bits, lo, hi), st
    assert (lo + hi) * bits >= 254 and (lo - 1) * bits // 2 + 1 <= 64
    assert st["sel_words"] <= 32, st  # the stream stays within the record's 32 scalar words
    assert st["fixed_cases"] == 15 and st["random_cases"] == 100000, st
    # the patterns did reach both ends of the digit range, several digits each
    assert st["fixed_min_digits"] >= lo and st["fixed_max_digits"] >= lo, st
    assert st["zero_digits"] > 0 and st["unit_digits"] > 0, st
