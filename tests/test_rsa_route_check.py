"""The routing geometry of K20 (corda_amd/csrc/rsa_route.hpp) on the host under AddressSanitizer +
UBSan: tools/rsa_route_check.cpp replays the gather of the live records, the match, the waves'
ballots, one reservation per list and wave and the ranked writes into buffers of exactly the sizes
the layout names, and compares them with a plain sequential partition -- the rule (width class,
exponent and all W modulus words; a cleared record whose modulus matches, the same key live twice,
records equal in n[0] and e that differ only in the top word or only in a middle word, equal n with
another e, a short key in a wider row; 0, 1 and 64 live records, all three classes and one only),
the keyed and generic lists and their counts for 1 to 513 rows (all keyed, none, alternating, a
keyed run across a block edge, random), rows the prep decided in neither list, the waves'
reservations in order and shuffled, the indexed kernels' grids over lists whose length only the
device knows, and the launch loop over workspace caps of 64, 128 and 4096 rows with counters fresh
per launch. A stand-alone program: nothing is loaded into Python."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_rsa_route_geometry_asan_ubsan(tmp_path):
    exe = str(tmp_path / "rsa_route_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "rsa_route_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20261021"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["failures"] == 0, st
    # 8 tables x 3 classes x 11 row counts x 5 patterns x 3 workspace caps, waves in order and shuffled
    assert st["tables"] == 8 and st["cases"] == 8 * 3 * 11 * 5 * 3 * 2, st
    assert st["keyed"] > 0 and st["rows"] > st["keyed"] and all(c > 0 for c in st["class_hits"]), st
    assert st["decided"] > 0 and st["dead_blocks"] > 0, st
    # the launch loop ran: 513 rows over a 64-row workspace are 9 launches
    assert st["multi_launch_cases"] > 0 and st["launches"] > st["cases"], st
    # the rule's corner cases were met. The 96-word key K is live in 5 of the 8 tables (one, three,
    # rel_k, dup, full) and cleared or absent in 3; its relatives TOP and MID are live in rel and rel_k
    assert st["cleared_misses"] == 3 and st["exp_misses"] == 5 and st["dup_hits"] == 1, st
    assert st["top_misses"] == 4 and st["mid_misses"] == 4 and st["short_misses"] == 4, st
