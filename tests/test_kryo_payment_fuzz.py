"""tools/kryo_fuzz.cpp (the mutation fuzzer of the Kryo encoder core, a stand-alone program
built with AddressSanitizer + UBSan as tests/test_kryo_fuzz.py builds it) over seeds of the
two kinds a payment adds -- MOVE_COMMAND in every shape of tests/test_kryo_payment.py and
SECURE_HASH -- and over the payment corpus' items (corda_amd.corpus.cash_payment_items), so
its "another kind" mutation also lands other payloads on kinds 18 and 19. It must exit 0 with
no sanitizer report, and the mutants must reach both sides: valid leaves, rejections and
template rebuilds."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from corda_amd import _lib
from corda_amd.corpus import cash_payment_items
from test_kryo_payment import HASH, move_cases, move_item

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(blob, arr):
    out = bytearray()
    blob = np.ascontiguousarray(blob)
    for it in arr:
        kind, ln, d = int(it["kind"]), int(it["len"]), int(it["data"])
        nb = 2 * ln if kind in (9, 12) else ln
        out += struct.pack("<IIqQQ", kind, int(it["class_id"]), int(it["value"]), ln, nb) + blob[d:d + nb].tobytes()
    return out


def _write_seeds(path):
    items = [move_item(c) for c in move_cases()] + [("secure_hash", HASH, 0), ("secure_hash", bytes(32), 0)]
    blob, arr, _ = _lib.kryo_pack(items)
    out = _records(blob, arr)
    r = np.random.default_rng(3)
    c = cash_payment_items(r.integers(0, 256, (8, 32), dtype=np.uint8), bytes(range(32)), 12, 5, window_frac=0.5)
    out += _records(c["blob"], c["items"])
    with open(path, "wb") as f:
        f.write(out)
    kinds = {int(k) for k in arr["kind"]} | {int(k) for k in c["items"]["kind"]}
    return len(items) + len(c["items"]), kinds


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ absent")
def test_payment_kinds_fuzz_asan_ubsan(tmp_path):
    exe = str(tmp_path / "kryo_fuzz")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tools", "kryo_fuzz.cpp"),
                           os.path.join(ROOT, "corda_amd", "csrc", "kryo.cpp"),
                           os.path.join(ROOT, "tools", "kryo_tmpl_check.cpp")])
    seeds = str(tmp_path / "seeds.bin")
    nseeds, kinds = _write_seeds(seeds)
    assert {10, 12, 13, 15, 16, 17, 18, 19} <= kinds  # every component kind of a payment, and the attachment id
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe, seeds, "3000", "20261021"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    # both sides: valid leaves and template rebuilds as well as rejections
    assert nseeds > 100 and st["items"] // 4 < st["valid"] < st["items"] and st["templated"] > 1000, st
