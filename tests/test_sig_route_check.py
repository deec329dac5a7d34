"""The counted route passes of K24 (the three families' route kernels with a row count read from
device memory) on the host under AddressSanitizer + UBSan: tools/sig_route_check.cpp replays them
wave by wave into buffers of exactly the sizes the layouts name for the host's bound and compares
them with a plain sequential partition of rows 0 .. count -- counts 0, 1, 63, 64, 65, bound - 1,
bound and counts above the bound (clipped), at the tile edges of each family (Ed25519 2,048 /
2,049, ECDSA 4,096 / 4,097, RSA 256 / 257 rows), the waves' reservations in order and shuffled:
no row at or past the count in any list, nothing written past a list's count, the totals as
expected. A stand-alone program: nothing is loaded into Python."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_counted_route_passes_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sig_route_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "sig_route_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20261021"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["failures"] == 0, st
    # 2 tables x 3 bounds x 9 counts x 4 row patterns, in order and shuffled; RSA over 2 workspaces
    per = 2 * 3 * 9 * 4 * 2
    assert st["ed_cases"] == per and st["ec_cases"] == per and st["rsa_cases"] == 2 * per, st
    # two of the nine counts are above the bound
    assert st["clipped_cases"] == (per + per + 2 * per) * 2 // 9, st
    assert st["keyed"] > 0 and st["rows_routed"] > st["keyed"] and st["rows_past"] > 0, st
    # RSA launches wholly past the count, and rows the prep decided, occurred
    assert st["empty_launches"] > 0 and st["decided"] > 0, st
