"""Mutation fuzzing of cordahip_verify_keyed's CSR validation and chunk packing under
AddressSanitizer + UBSan (host only): tools/vkey_csr_fuzz.cpp builds keyed batches with
every array in a heap block of exactly its declared entries, mutates sig_off, msg_off,
sig_bytes, msg_bytes and n, and checks that check_keyed_sig_batch (csr_check.hpp) fails
exactly the batches the contract rejects -- and that a batch it accepts is packed chunk by
chunk (pack_rows.hpp msg_chunk_layout / keyed_pack_rows, the code cordahip_verify_keyed
runs) into exact-size stages without a read outside a caller buffer or a write outside a
stage, with the statuses the host decides (EMPTY, MALFORMED_SIG) as the contract states. Every
accepted batch also goes through cordahip_rsa_verify_keyed's packer (rsa_keyed_msg_offsets /
rsa_keyed_pack_rows): lanes grouped by a random width class, small launches, exact-size stages,
every row compared with its lane."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_vkey_csr_fuzz_asan_ubsan(tmp_path):
    exe = str(tmp_path / "vkey_csr_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "vkey_csr_fuzz.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, "20000", "20261019"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["batches"] == 20000
    # both verdicts occur in more than 10 % of the batches; both chunk layouts were packed
    assert 2000 < st["invalid"] < st["batches"] - 2000, st
    assert st["dense_chunks"] > 1000 and st["csr_chunks"] > 1000 and st["empty_msgs"] > 1000, st
    # every host-decided status occurred
    assert st["pre_ok"] > 10000 and st["pre_empty"] > 1000 and st["pre_malformed"] > 1000, st
    assert st["lanes_packed"] > 100000, st
    # the RSA walk ran: rows of every width class, lanes left out as unknown ids, signatures longer
    # than their slot, slot-edge lengths (0, 4 W - 1, 4 W, 4 W + 1) and empty messages (floors a third
    # or less of what the committed seed gives: they keep the walk exercised, they measure nothing)
    assert len(st["rsa_rows"]) == 3 and all(x > 50000 for x in st["rsa_rows"]), st
    assert st["rsa_launches"] > 30000 and st["rsa_unknown"] > 50000, st
    assert st["rsa_oversize"] > 10000 and st["rsa_edge_lens"] > 10000 and st["rsa_empty_msgs"] > 10000, st
