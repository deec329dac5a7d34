"""The commit log's removal (corda_amd/csrc/commit_core.hpp: erase_at, erase_row and the
per-cluster repair_cluster -- the code cordahip_commit_log_revoke's kernels run) on the host under
AddressSanitizer + UBSan: tools/commit_erase_check.cpp interleaves loads, run_serial batches,
erase_row calls and whole revokes (row by row against mark + per-cluster repair in shuffled
order) over a 64-slot table in a heap block of exactly its size against a std::map, and checks
the whole universe and the table's structure after every step. A stand-alone program: nothing is
loaded into Python.

With the committed seed (3000 rounds, seed 20261020) the program reports
  removals 6278, refused_id 1673, refused_index 1712, refused_caller 1705, refused_absent 17688,
  wrap_shifts 66 (an entry moved back across the table's end), erased_cluster_starts 3010,
  cluster_splits 1312, revokes 12312 (revoke_removed 24122), adjacent_marked 1445,
  wrapping_clusters_repaired 828, max_entries 53;
the floors below are half of those."""
import json
import os
import shutil
import struct
import subprocess

import pytest

from commit_revoke_model import hash_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ absent")
    out = str(tmp_path_factory.mktemp("erase") / "commit_erase_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", out,
                           os.path.join(ROOT, "tools", "commit_erase_check.cpp")])
    return out


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_erase_against_map_model_asan_ubsan(exe):
    p = subprocess.run([exe, "3000", "20261020"], capture_output=True, text=True, env=ENV, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] is True and st["failures"] == 0 and st["rounds"] == 3000, st
    floors = {"removals": 3139, "refused_id": 836, "refused_index": 856, "refused_caller": 852,
              "refused_absent": 8844, "wrap_shifts": 33, "erased_cluster_starts": 1505, "cluster_splits": 656,
              "revokes": 6156, "revoke_removed": 12061, "adjacent_marked": 722, "wrapping_clusters_repaired": 414}
    for k, floor in floors.items():
        assert st[k] >= floor, (k, st)
    assert 50 <= st["max_entries"] <= 56, st  # the table ran near 7/8 of its 64 slots


def test_python_siphash_is_the_cores(exe):
    p = subprocess.run([exe, "--hash"], capture_output=True, text=True, env=ENV, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    cases = json.loads(p.stdout)
    assert len(cases) == 4
    for c in cases:
        ref = (struct.pack("<8I", *c["ref"][:8]), c["ref"][8])
        assert hash_ref(ref, c["k0"], c["k1"]) == c["hash"], c
