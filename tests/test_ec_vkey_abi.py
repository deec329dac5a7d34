"""The keyed ECDSA entry points at the drop-in boundary (CPU-only): the four new functions are
declared in include/cordahip.h with the argument lists the ctypes bindings use, are exported by
the library, leave the ABI version at 4, and answer CORDAHIP_ERR_INVALID_ARG without a context
or a batch; the geometry header's table size is the one the header documents."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NEW = {"cordahip_vkey_add_ecdsa": 6, "cordahip_ecdsa_verify_keyed": 2, "cordahip_ecdsa_verify_keyed_submit": 3,
       "cordahip_ecdsa_verify_keyed_device": 11}


@pytest.fixture(scope="module")
def lib():
    from corda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "corda_amd", "csrc")])
    return _lib.lib()


def test_new_entry_points_declared_bound_and_exported(lib):
    from corda_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "#define CORDAHIP_ABI_VERSION 4u" in src and _lib.ABI_VERSION == 4
    for f, nargs in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % f, src)
        assert m, f
        assert len(m.group(1).split(",")) == nargs, f  # the header's argument count ...
        assert f in _lib.EXPORTS and getattr(lib, f) is not None, f
        assert len(getattr(lib, f).argtypes) == nargs, f  # ... is the binding's
        assert getattr(lib, f).restype is ctypes.c_int32 or getattr(lib, f).restype is ctypes.c_int, f
    # the batch struct is the Ed25519 keyed call's
    assert re.search(r"cordahip_ecdsa_verify_keyed\s*\(\s*cordahip_ctx\s*\*\s*ctx,\s*const\s+cordahip_keyed_sig_batch\s*\*", src)


def test_geometry_matches_header_text():
    geo = open(os.path.join(ROOT, "corda_amd", "csrc", "ecdsa_vkey.hpp")).read()
    assert re.search(r"kEcVkeyEntryWords = 20;", geo) and "320u * 1024u" in geo
    doc = open(HEADER).read()
    assert "(320 KiB)" in doc and "ONE pool of CORDAHIP_VKEY_MAX_KEYS" in doc


def test_null_context_or_batch_is_invalid_arg(lib):
    from corda_amd import _lib
    key, kid, st, t = bytes(65), ctypes.c_uint32(), ctypes.c_uint8(), ctypes.c_uint64()
    b = _lib.KeyedSigBatch()
    assert lib.cordahip_vkey_add_ecdsa(None, 3, key, 65, ctypes.byref(kid), ctypes.byref(st)) == -1
    assert lib.cordahip_ecdsa_verify_keyed(None, ctypes.byref(b)) == -1
    assert lib.cordahip_ecdsa_verify_keyed(None, None) == -1
    assert lib.cordahip_ecdsa_verify_keyed_submit(None, ctypes.byref(b), ctypes.byref(t)) == -1
    assert lib.cordahip_ecdsa_verify_keyed_submit(None, None, None) == -1
    assert lib.cordahip_ecdsa_verify_keyed_device(None, 0, None, None, None, None, 32, 0, None, None, None) == -1
