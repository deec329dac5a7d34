"""The commit log's entry points at the drop-in boundary (CPU-only): the four new structs as
ctypes lays them out against the C compiler's layout of include/cordahip.h (the method of
tests/test_abi.py), the numpy row images, the new status and error values against the header
and the kernel's constants, and every new entry point answering CORDAHIP_ERR_INVALID_ARG
without a context."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NEW = ["cordahip_commit_log_create", "cordahip_commit_log_destroy", "cordahip_commit_log_reserve",
       "cordahip_commit_log_stats", "cordahip_commit_log_load", "cordahip_commit_log_lookup",
       "cordahip_commit_inputs", "cordahip_commit_inputs_submit", "cordahip_commit_inputs_device"]


@pytest.fixture(scope="module")
def lib():
    from corda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "corda_amd", "csrc")])
    return _lib.lib()


def test_commit_struct_layouts_match_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc absent")
    from corda_amd import _lib
    structs = {"cordahip_state_ref": _lib.StateRef, "cordahip_consuming_tx": _lib.ConsumingTx,
               "cordahip_commit_row": _lib.CommitRow, "cordahip_commit_batch": _lib.CommitBatch}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cordahip.h"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, (cname, f[0])
    # the row sizes the header states, and the numpy images of the rows
    assert (int(got["cordahip_state_ref"]), int(got["cordahip_consuming_tx"]), int(got["cordahip_commit_row"])) == \
        (36, 40, 76)
    assert (_lib.STATE_REF_DTYPE.itemsize, _lib.CONSUMING_TX_DTYPE.itemsize, _lib.COMMIT_ROW_DTYPE.itemsize) == \
        (36, 40, 76)
    assert _lib.STATE_REF_DTYPE.fields["index"][1] == _lib.StateRef.index.offset
    assert _lib.CONSUMING_TX_DTYPE.fields["input_index"][1] == _lib.ConsumingTx.input_index.offset
    assert _lib.CONSUMING_TX_DTYPE.fields["caller"][1] == _lib.ConsumingTx.caller.offset
    assert _lib.COMMIT_ROW_DTYPE.fields["by"][1] == _lib.CommitRow.by.offset
    assert [f[0] for f in _lib.CommitBatch._fields_] == [
        "ntx", "txid", "caller", "refs", "tx_ref_off", "n_refs", "tw_from", "tw_until", "now_ns", "tolerance_ns",
        "gate", "tx_status", "committed", "ref_state", "ref_by"]
    assert ctypes.sizeof(_lib.CommitBatch) == 15 * 8


def test_commit_values_match_header():
    from corda_amd import _lib, resolve
    src = open(HEADER).read()
    vals = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define CORDAHIP_COMMIT_(\w+) (\d+)", src))
    assert vals == {"CONFLICT": _lib.COMMIT_CONFLICT, "TIME_WINDOW_INVALID": _lib.COMMIT_TIME_WINDOW_INVALID,
                    "SKIPPED": _lib.COMMIT_SKIPPED} == {"CONFLICT": 16, "TIME_WINDOW_INVALID": 17, "SKIPPED": 18}
    assert (resolve._COMMIT_CONFLICT, resolve._COMMIT_TIME_WINDOW_INVALID) == (16, 17)
    assert re.search(r"#define CORDAHIP_ERR_LOG_FULL \(-9\)", src) and _lib.ERR_LOG_FULL == -9
    assert "#define CORDAHIP_ABI_VERSION 4u" in src
    # no transaction status of the header has these values (they share tx_status arrays with them)
    others = [int(v) for v in re.findall(r"#define CORDAHIP_(?:STATUS|TX)_\w+ (\d+)", src)]
    assert len(others) > 10 and not {16, 17, 18} & set(others)
    # the kernel's constants (commit_core.hpp) are the header's, and the model's
    core = open(os.path.join(ROOT, "corda_amd", "csrc", "commit_core.hpp")).read()
    assert re.search(r"kCommitOk = 0, kCommitConflict = 16, kCommitTimeWindowInvalid = 17, kCommitSkipped = 18;", core)
    assert re.search(r"kRefAbsent = 0, kRefSelf = 1, kRefOther = 2;", core)
    import commit_log_model as model
    assert (model.COMMIT_CONFLICT, model.COMMIT_TIME_WINDOW_INVALID, model.COMMIT_SKIPPED) == (16, 17, 18)
    assert (model.REF_ABSENT, model.REF_SELF, model.REF_OTHER) == (_lib.REF_ABSENT, _lib.REF_SELF, _lib.REF_OTHER)
    assert _lib.TW_SIDE_ABSENT == -(1 << 63) and _lib.TW_SATURATE == 1 << 62


def test_new_entry_points_declared_and_exported(lib):
    from corda_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, src), f
        assert f in _lib.EXPORTS and getattr(lib, f) is not None, f


def test_strerror_names_the_full_log(lib):
    assert lib.cordahip_strerror(-9) == b"commit log full (reserve a larger capacity)"


def test_null_context_is_invalid_arg(lib):
    from corda_amd import _lib
    lid, t, n = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
    b = _lib.CommitBatch()
    row, r = _lib.CommitRow(), _lib.StateRef()
    present, by = ctypes.c_uint8(), _lib.ConsumingTx()
    assert lib.cordahip_commit_log_create(None, 0, 10, None, ctypes.byref(lid)) == -1
    assert lib.cordahip_commit_log_destroy(None, 1) == -1
    assert lib.cordahip_commit_log_reserve(None, 1, 12) == -1
    assert lib.cordahip_commit_log_stats(None, 1, ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.cordahip_commit_log_load(None, 1, ctypes.byref(row), 1, ctypes.byref(n)) == -1
    assert lib.cordahip_commit_log_lookup(None, 1, ctypes.byref(r), 1, ctypes.byref(present), ctypes.byref(by)) == -1
    assert lib.cordahip_commit_inputs(None, 1, ctypes.byref(b)) == -1
    assert lib.cordahip_commit_inputs(None, 1, None) == -1
    assert lib.cordahip_commit_inputs_submit(None, 1, ctypes.byref(b), ctypes.byref(t)) == -1
    assert lib.cordahip_commit_inputs_submit(None, 1, None, None) == -1
    assert lib.cordahip_commit_inputs_device(None, 1, ctypes.byref(b), None) == -1
    assert lib.cordahip_commit_inputs_device(None, 1, None, None) == -1
