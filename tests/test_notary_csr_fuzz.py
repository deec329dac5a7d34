"""Mutation fuzzing of cordahip_notary_tearoff_*'s validation under AddressSanitizer + UBSan (host
only): tools/notary_csr_fuzz.cpp builds typed tear-off batches with every array in a heap block of
exactly its declared entries, mutates tx_ref_off, tx_tok_off, n_refs, ntok, the transaction count
and the NULL pairing of the five window arrays, and checks that check_notary_tearoff
(csr_check.hpp) accepts exactly what an independent statement of the contract accepts -- and that
every leaf an accepted batch names (refs in list order, then the window, formed as K21 forms its
items) runs through the host instance of the encoder (kryo_core.hpp) without a read outside a
caller array, window rows being valid exactly when the header's rule says so."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_notary_csr_fuzz_asan_ubsan(tmp_path):
    exe = str(tmp_path / "notary_csr_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "notary_csr_fuzz.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "6000", "20261021"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["batches"] == 6000, st
    # both verdicts occur in more than 10 % of the batches; the accepted ones ran
    assert 600 < st["invalid"] < st["batches"] - 600, st
    assert st["ran"] == st["batches"] - st["invalid"], st
    assert st["txs"] > 30000 and st["ref_leaves"] > 50000 and st["window_leaves"] > 5000 and st["bad_windows"] > 500, st
