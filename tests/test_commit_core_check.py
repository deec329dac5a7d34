"""The commit log's core (corda_amd/csrc/commit_core.hpp: keyed slot index, linear probing, the
time-window rule, the in-order commit and the report -- the code the K16 kernels run) on the
host under AddressSanitizer + UBSan: tools/commit_core_check.cpp runs seeded batches (refs from
40 values, 8 transaction ids, 3 callers, gates, windows at and one ns past the tolerance) over a
64-slot table in a heap block of exactly its size, at up to 7/8 load, against an independent
std::map model, and looks the whole universe up after every batch. A stand-alone program:
nothing is loaded into Python."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_commit_core_against_map_model_asan_ubsan(tmp_path):
    exe = str(tmp_path / "commit_core_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "commit_core_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "3000", "20261020"], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["failures"] == 0 and st["rounds"] == 3000, st
    # every outcome occurred, in numbers
    assert st["batches"] > 10000 and st["txs"] > 100000, st
    for k in ("committed", "conflicts", "skipped", "window_invalid"):
        assert st[k] > 5000, (k, st)
    assert st["already"] > 100 and st["loads_dup"] > 1000, st
    # the table ran near 7/8 of its 64 slots and probes wrapped its end
    assert 50 <= st["max_entries"] <= 56 and st["wrapped"] > 1000, st
