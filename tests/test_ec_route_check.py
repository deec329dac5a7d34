"""The routing geometry of K15 (corda_amd/csrc/ecdsa_route.hpp) on the host under
AddressSanitizer + UBSan: tools/ec_route_check.cpp replays the gather, route, count and
scatter passes wave by wave into buffers of exactly the sizes the layout names and compares
them with a plain sequential partition -- the match rule (both SEC1 encodings of a registered
point; the wrong parity, another Y, the other scheme byte, hybrid prefixes and key lengths 1,
33, 64 and 65; records with an equal first X word and different tails, a dead record whose
point matches, the same point live twice; 0, 1 and 64 live keys, both curves and one only),
the seven class runs of perm and their counts at wave, block and tile edges, with the waves'
range reservations in order and shuffled, and the generic engine's workspace chunks over a
list whose length only the device knows. A stand-alone program: nothing is loaded into Python."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_ec_route_geometry_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ec_route_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ec_route_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20261020"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["failures"] == 0, st
    # 9 tables x 12 lane counts x 6 patterns, each with the waves in order and shuffled
    assert st["tables"] == 9 and st["cases"] == 9 * 12 * 6 * 2, st
    assert st["keyed"] > 0 and st["lanes"] > st["keyed"] and st["keyed_k1"] > 0 and st["keyed_r1"] > 0, st
    # the rule's corner cases were met. Probes run per table and scheme byte (18): the point K is
    # live under scheme 2 in 5 tables (one, both, tails_k, dup, full) and under scheme 3 in one
    assert st["unc_hits"] == 6 and st["comp_hits"] == 6 and st["dead_misses"] == 12, st
    assert st["scheme_misses"] == 6 and st["parity_misses"] == 6 and st["negy_misses"] == 6, st
    assert st["len_misses"] == 18 * 7 and st["tail_misses"] >= 12 and st["dup_hits"] == 1, st
    # every case with the seven counts right checked 4 workspace sizes; chunks wholly past the count occurred
    assert st["chunk_cases"] == 4 * st["cases"] and st["empty_chunks"] > 0, st
