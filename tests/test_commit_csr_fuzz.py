"""Mutation fuzzing of cordahip_commit_inputs' validation under AddressSanitizer + UBSan (host
only): tools/commit_csr_fuzz.cpp builds commit batches with every array in a heap block of
exactly its declared entries, mutates tx_ref_off, n_refs, the transaction count, now_ns,
tolerance_ns and the pairing of the window arrays, and checks that check_commit (csr_check.hpp)
accepts exactly what an independent statement of the contract accepts -- and that an accepted
batch runs through the host instance of the commit core (commit_core.hpp) without a read
outside a caller array, a write outside an output, or an overflowing time difference (window
sides at the saturation bounds, now and tolerance at the ends of their ranges)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_commit_csr_fuzz_asan_ubsan(tmp_path):
    exe = str(tmp_path / "commit_csr_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "commit_csr_fuzz.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20000", "20261020"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["batches"] == 20000, st
    # both verdicts occur in more than 10 % of the batches; the accepted ones ran
    assert 2000 < st["invalid"] < st["batches"] - 2000, st
    assert st["ran"] == st["batches"] - st["invalid"], st
    assert st["txs"] > 100000 and st["refs"] > 100000 and st["committed"] > 10000, st
    assert st["window_invalid"] > 10000 and st["edge_scalars"] > 1000, st
