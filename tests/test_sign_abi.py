"""The signing entry points at the drop-in boundary (CPU-only): cordahip_sign_batch as
ctypes lays it out against the C compiler's layout of include/cordahip.h (the method of
tests/test_abi.py), the new status values against the header, and every new entry
point answering CORDAHIP_ERR_INVALID_ARG without a context."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NEW = ["cordahip_signer_add_ed25519", "cordahip_signer_remove", "cordahip_sign", "cordahip_sign_submit",
       "cordahip_ed25519_sign_keyed_device"]


@pytest.fixture(scope="module")
def lib():
    from corda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "corda_amd", "csrc")])
    return _lib.lib()


def test_sign_batch_layout_matches_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc absent")
    from corda_amd import _lib
    cls, cname = _lib.SignBatch, "cordahip_sign_batch"
    assert [f[0] for f in cls._fields_] == ["n", "key_id", "msg", "msg_off", "gate", "sig", "status", "msg_bytes"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cordahip.h"', "int main(void) {",
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls) == 64
    for f in cls._fields_:
        assert int(got["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]


def test_sign_statuses_match_header():
    from corda_amd import _lib, resolve
    src = open(HEADER).read()
    vals = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"#define CORDAHIP_SIGN_(\w+) (\d+)", src))
    assert vals == {"UNKNOWN_KEY": _lib.SIGN_UNKNOWN_KEY, "SKIPPED": _lib.SIGN_SKIPPED} == {"UNKNOWN_KEY": 14,
                                                                                             "SKIPPED": 15}
    assert resolve._SIGN_UNKNOWN_KEY == _lib.SIGN_UNKNOWN_KEY
    # no other status of the header has these values
    others = [int(v) for v in re.findall(r"#define CORDAHIP_(?:STATUS|TX)_\w+ (\d+)", src)]
    assert not {14, 15} & set(others) and "#define CORDAHIP_ABI_VERSION 4u" in src
    # the kernel's constants (status.hpp) are the header's
    st = open(os.path.join(ROOT, "corda_amd", "csrc", "status.hpp")).read()
    assert re.search(r"kSignUnknownKey = 14;", st) and re.search(r"kSignSkipped = 15;", st)
    # the registry's capacity as documented
    assert _lib.SIGNER_MAX_KEYS == 4096 and "up to 4096 live keys" in src


def test_new_entry_points_declared_and_exported(lib):
    from corda_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, src), f
        assert f in _lib.EXPORTS and getattr(lib, f) is not None, f


def test_null_context_is_invalid_arg(lib):
    from corda_amd import _lib
    seed, pub, kid, t = bytes(32), ctypes.create_string_buffer(32), ctypes.c_uint32(), ctypes.c_uint64()
    b = _lib.SignBatch()
    assert lib.cordahip_signer_add_ed25519(None, seed, ctypes.byref(kid), pub) == -1
    assert lib.cordahip_signer_remove(None, 0) == -1
    assert lib.cordahip_sign(None, ctypes.byref(b)) == -1
    assert lib.cordahip_sign(None, None) == -1
    assert lib.cordahip_sign_submit(None, ctypes.byref(b), ctypes.byref(t)) == -1
    assert lib.cordahip_sign_submit(None, None, None) == -1
    assert lib.cordahip_ed25519_sign_keyed_device(None, 0, None, None, 32, 0, None, None, None, None) == -1
