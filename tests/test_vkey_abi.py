"""The keyed-verification entry points at the drop-in boundary (CPU-only):
cordahip_keyed_sig_batch as ctypes lays it out against the C compiler's layout of
include/cordahip.h (the method of tests/test_sign_abi.py), the new status value against
the header and status.hpp, and every new entry point answering CORDAHIP_ERR_INVALID_ARG
without a context or a batch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NEW = ["cordahip_vkey_add_ed25519", "cordahip_vkey_remove", "cordahip_verify_keyed", "cordahip_verify_keyed_submit",
       "cordahip_ed25519_verify_keyed_device"]
FIELDS = ["n", "key_id", "sig", "sig_off", "msg", "msg_off", "status", "verdict", "flags", "sig_bytes", "msg_bytes"]


@pytest.fixture(scope="module")
def lib():
    from corda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "corda_amd", "csrc")])
    return _lib.lib()


def test_keyed_sig_batch_layout_matches_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc absent")
    from corda_amd import _lib
    cls, cname = _lib.KeyedSigBatch, "cordahip_keyed_sig_batch"
    assert [f[0] for f in cls._fields_] == FIELDS
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
    assert int(got[cname]) == ctypes.sizeof(cls) == 88
    for f in cls._fields_:
        assert int(got["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]


def test_unknown_key_status_matches_header():
    from corda_amd import _lib, resolve
    src = open(HEADER).read()
    m = re.search(r"#define CORDAHIP_VERIFY_UNKNOWN_KEY (\d+)", src)
    assert m and int(m.group(1)) == _lib.VERIFY_UNKNOWN_KEY == resolve._VERIFY_UNKNOWN_KEY == 16
    # no other status of the header has this value
    others = [int(v) for v in re.findall(r"#define CORDAHIP_(?:STATUS|TX|SIGN|REQ)_\w+ (\d+)", src)]
    assert len(others) > 10 and 16 not in others and "#define CORDAHIP_ABI_VERSION 4u" in src
    # the kernel's constant (status.hpp) is the header's
    st = open(os.path.join(ROOT, "corda_amd", "csrc", "status.hpp")).read()
    assert re.search(r"kVerifyUnknownKey = 16;", st)
    # the registry's capacity: header, Python and the geometry header agree
    cap = re.search(r"#define CORDAHIP_VKEY_MAX_KEYS (\d+)", src)
    geo = open(os.path.join(ROOT, "corda_amd", "csrc", "ed25519_vkey.hpp")).read()
    bits = re.search(r"kVkeySlotBits = (\d+);", geo)
    assert cap and bits and int(cap.group(1)) == _lib.VKEY_MAX_KEYS == 1 << int(bits.group(1))
    assert _lib.VKEY_NO_ID == 0xFFFFFFFF


def test_new_entry_points_declared_and_exported(lib):
    from corda_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, src), f
        assert f in _lib.EXPORTS and getattr(lib, f) is not None, f


def test_null_context_or_batch_is_invalid_arg(lib):
    from corda_amd import _lib
    key, kid, st, t = bytes(32), ctypes.c_uint32(), ctypes.c_uint8(), ctypes.c_uint64()
    b = _lib.KeyedSigBatch()
    assert lib.cordahip_vkey_add_ed25519(None, key, ctypes.byref(kid), ctypes.byref(st)) == -1
    assert lib.cordahip_vkey_remove(None, 0) == -1
    assert lib.cordahip_verify_keyed(None, ctypes.byref(b)) == -1
    assert lib.cordahip_verify_keyed(None, None) == -1
    assert lib.cordahip_verify_keyed_submit(None, ctypes.byref(b), ctypes.byref(t)) == -1
    assert lib.cordahip_verify_keyed_submit(None, None, None) == -1
    assert lib.cordahip_ed25519_verify_keyed_device(None, 0, None, None, None, 32, 0, None, None, None) == -1
