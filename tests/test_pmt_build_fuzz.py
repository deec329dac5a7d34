"""Mutation fuzzing of the FilteredTransaction build under AddressSanitizer + UBSan
(host only): tools/pmt_build_fuzz.cpp builds batches with every array in a heap
block of exactly its declared size, mutates offsets, slot sizes, declared counts,
transaction sizes, duplicate leaf hashes and masks, checks that
check_filtered_build_batch (csr_check.hpp) rejects exactly what the contract
rejects, and runs the core the GPU kernel runs (pmt_core.hpp, with a stand-in
node hash) lane by lane against an independent recursive build."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_pmt_build_fuzz_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pmt_build_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "pmt_build_fuzz.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "8000", "20261019"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    # both verdicts of the validation, and every status the core can produce
    assert 0 < st["invalid"] < st["batches"], st
    for k in ("status_0", "status_6", "status_12", "status_13"):
        assert st[k] > 100, st
    assert st["lanes"] > 10000 and st["tokens"] > 100000, st
