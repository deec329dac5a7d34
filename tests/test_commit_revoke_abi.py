"""cordahip_commit_log_revoke and cordahip_commit_log_export at the drop-in boundary (CPU-only):
declared in include/cordahip.h, exported and bound, CORDAHIP_ERR_INVALID_ARG without a context,
and no new status value or ABI version with them."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NEW = ["cordahip_commit_log_revoke", "cordahip_commit_log_export"]


@pytest.fixture(scope="module")
def lib():
    from corda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "corda_amd", "csrc")])
    return _lib.lib()


def test_declared_exported_and_bound(lib):
    from corda_amd import _lib
    from corda_amd.engine import Engine
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for f in NEW:
        assert re.search(r"\bint %s\s*\(cordahip_ctx\* ctx, uint32_t log_id," % f, src), f
        assert f in _lib.EXPORTS and getattr(lib, f).argtypes is not None, f
    assert callable(Engine.commit_log_revoke) and callable(Engine.commit_log_export)
    from corda_amd import resolve
    assert callable(resolve.notarise_filtered_transactions_persisted)


def test_null_context_is_invalid_arg(lib):
    from corda_amd import _lib
    row, rev, n = _lib.CommitRow(), ctypes.c_uint8(7), ctypes.c_uint64(7)
    seq = ctypes.c_uint64(7)
    assert lib.cordahip_commit_log_revoke(None, 1, ctypes.byref(row), 1, ctypes.byref(rev), ctypes.byref(n)) == -1
    assert lib.cordahip_commit_log_revoke(None, 1, None, 0, None, None) == -1
    assert lib.cordahip_commit_log_export(None, 1, 0, ctypes.byref(row), ctypes.byref(seq), 1, ctypes.byref(n)) == -1
    assert lib.cordahip_commit_log_export(None, 1, 0, None, None, 0, None) == -1
    assert (rev.value, n.value, seq.value) == (7, 7, 7)  # nothing written


def test_no_new_status_and_the_same_abi():
    src = open(HEADER).read()
    assert sorted(re.findall(r"#define (CORDAHIP_COMMIT_\w+)", src)) == [
        "CORDAHIP_COMMIT_CONFLICT", "CORDAHIP_COMMIT_SKIPPED", "CORDAHIP_COMMIT_TIME_WINDOW_INVALID"]
    assert "#define CORDAHIP_ABI_VERSION 4u" in src
    # the header says what the order of an export is, and where a sequence number comes from
    doc = re.search(r"/\* Export:.*?\*/", src, flags=re.S).group(0)
    assert "ORDER OF THE ROWS IS UNSPECIFIED" in doc and "next_seq" in doc
