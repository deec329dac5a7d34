"""Mutation fuzzing of the required-signer coverage core under AddressSanitizer +
UBSan (host only): tools/cover_fuzz.cpp builds cordahip_cover batches with every
array in a heap block of exactly its declared entries, mutates offsets, declared
counts and token fields, and checks that check_cover (csr_check.hpp) rejects
exactly the batches the contract rejects, and that a batch it accepts is
evaluated by cover_core.hpp -- with the host workers' stack, the kernel's
per-token slice and the dense-row key reader -- to the verdicts of an
independent recursive evaluator, without a read or write outside any buffer."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_cover_fuzz_asan_ubsan(tmp_path):
    exe = str(tmp_path / "cover_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "cover_fuzz.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20000", "20261019"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    # both verdicts of the CSR check occur, and the accepted batches reach every outcome
    assert 0 < st["invalid"] < st["batches"] == 20000, st
    assert st["dense_batches"] > 1000 and st["txs"] > 50000, st
    for k in ("tx_ok", "tx_missing", "tx_bad_cover", "tx_kept", "req_fulfilled", "req_missing", "req_allowed",
              "req_not_evaluated", "req_malformed"):
        assert st[k] > 1000, (k, st)
