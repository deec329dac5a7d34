"""The K22 extraction rule (corda_amd/csrc/txcomp_inputs_core.hpp: what the kernels of
cordahip_txcomp_inputs_device run) on the CPU under AddressSanitizer + UBSan:
tools/txcomp_inputs_check.cpp, a stand-alone program, drives it over fuzzed item arrays --
kinds, lengths, payload offsets beyond the payload, item offsets beyond n_items, ref_cap
from 0 to more than needed -- with every array in a heap block of exactly its size, and
compares the outputs with a plain re-statement of the rule."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_txcomp_inputs_core_asan_ubsan(tmp_path):
    exe = str(tmp_path / "txcomp_inputs_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "txcomp_inputs_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20000", "20261021"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    # the batches reach every side of the rule
    assert st["txs"] > 50000 and st["refs"] > 20000 and st["windows"] > 1000, st
    assert st["flagged"] > 1000 and st["capped"] > 1000, st
