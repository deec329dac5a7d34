"""The key registries' slot bookkeeping on the CPU under AddressSanitizer + UBSan:
tools/key_slots_check.cpp includes corda_amd/csrc/key_slots.hpp (no HIP) and runs KeySlots
in the verification keys' geometry (6 slot bits, counters 1 .. kVkeyGenMax) and the
signer's (12 slot bits, counters modulo 2^20): capacity and the full report, distinct ids,
slot reuse under a new id, rejection of released, stale and never-issued ids and of
kVkeyNoId with the count unchanged, a failed add's consumed counter, and both wraps."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_key_slots_asan_ubsan(tmp_path):
    exe = str(tmp_path / "key_slots_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tools", "key_slots_check.cpp"), "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    # one id per slot and the victim slot's second key, all distinct
    assert st == {"vkey_ids": 64 + 1, "signer_ids": 4096 + 1}, st
