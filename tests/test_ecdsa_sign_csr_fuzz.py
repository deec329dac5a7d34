"""Mutation fuzzing of cordahip_ecdsa_sign's CSR validation and chunk packing under
AddressSanitizer + UBSan (host only), as tests/test_sign_csr_fuzz.py does for
cordahip_sign: tools/ecdsa_sign_csr_fuzz.cpp builds ECDSA signing batches
(cordahip_ecdsa_sign_batch) with every array in a heap block of exactly its declared
entries, mutates msg_off, msg_bytes and n, and checks that check_sign_batch
(csr_check.hpp, the batch type a template parameter) fails exactly the batches the
contract rejects -- and that a batch it accepts is packed chunk by chunk
(pack_rows.hpp msg_chunk_layout / sign_pack_rows, the code cordahip_ecdsa_sign runs)
into exact-size stages without a read outside a caller buffer or a write outside a
stage."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_ecdsa_sign_csr_fuzz_asan_ubsan(tmp_path):
    exe = str(tmp_path / "ecdsa_sign_csr_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "ecdsa_sign_csr_fuzz.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20000", "20261020"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["batches"] == 20000
    # both verdicts occur, both chunk layouts were packed, empty messages among them
    assert 2000 < st["invalid"] < st["batches"] - 2000, st
    assert st["dense_chunks"] > 1000 and st["csr_chunks"] > 1000 and st["empty_msgs"] > 1000, st
    assert st["lanes_packed"] > 100000, st
