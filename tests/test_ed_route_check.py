"""The routing geometry of K14 (corda_amd/csrc/ed25519_route.hpp) on the host under
AddressSanitizer + UBSan: tools/ed_route_check.cpp replays the partition pass wave by wave
into a scratch of exactly the size the runtime allocates and compares it with a plain
sequential partition -- the match rule (records with equal first words and different tails,
a dead record whose bytes match, the same bytes live in two slots; 0, 1 and 64 live keys),
the two index lists and their counts at wave, block and tile edges, with the waves' range
reservations in order and shuffled, and the generic engine's workspace chunks over a list
whose length only the device knows. A stand-alone program: nothing is loaded into Python."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_route_geometry_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ed_route_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ed_route_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20261020"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["failures"] == 0, st
    # 7 tables x 12 lane counts x 6 patterns, each with the waves in order and shuffled
    assert st["tables"] == 7 and st["cases"] == 7 * 12 * 6 * 2, st
    assert st["keyed"] > 0 and st["lanes"] > st["keyed"], st
    # the rule's corner cases were met: K dead or absent in 3 tables (none, dead, tails), a tail
    # relative missing, duplicate bytes served by one of their two slots
    assert st["dead_misses"] == 3 and st["tail_misses"] >= 4 and st["dup_hits"] == 1, st
    # every case with both counts right checked 4 workspace sizes; chunks wholly past the count occurred
    assert st["chunk_cases"] == 4 * st["cases"] and st["empty_chunks"] > 0, st
