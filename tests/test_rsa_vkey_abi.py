"""The keyed RSA entry points at the drop-in boundary (CPU-only): the five new functions are
declared in include/cordahip.h with the argument lists the ctypes bindings use, are exported by
the library, leave the ABI version at 4, and answer CORDAHIP_ERR_INVALID_ARG without a context,
a batch or a key; the record header's table size is the one the header documents."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NEW = {"cordahip_vkey_add_rsa": 5, "cordahip_rsa_verify_keyed": 2, "cordahip_rsa_verify_keyed_submit": 3,
       "cordahip_rsa_verify_keyed_device": 12, "cordahip_rsa_public_op_keyed_device": 8}


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
    assert lib.cordahip_abi_version() == 4
    for f, nargs in NEW.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % f, src)
        assert m, f
        assert len(m.group(1).split(",")) == nargs, f  # the header's argument count ...
        assert f in _lib.EXPORTS and getattr(lib, f) is not None, f
        assert len(getattr(lib, f).argtypes) == nargs, f  # ... is the binding's
        assert getattr(lib, f).restype is ctypes.c_int32 or getattr(lib, f).restype is ctypes.c_int, f
    # the batch struct is the Ed25519 keyed call's
    assert re.search(r"cordahip_rsa_verify_keyed\s*\(\s*cordahip_ctx\s*\*\s*ctx,\s*const\s+cordahip_keyed_sig_batch\s*\*", src)


def test_record_size_matches_header_text():
    from corda_amd import _lib
    rec = open(os.path.join(ROOT, "corda_amd", "csrc", "rsa_vkey.hpp")).read()
    assert "sizeof(VkeyRecord) == 1056" in rec and "kVkeyTableBytes == 67584" in rec
    doc = open(HEADER).read()
    assert "67,584 bytes per device" in doc and re.search(r"1,056[\s*]+bytes", doc)
    assert "one id space for all three families" in doc
    assert _lib.RSA_VKEY_TABLE_BYTES == 67584 == _lib.VKEY_MAX_KEYS * 1056


def test_null_context_batch_or_key_is_invalid_arg(lib):
    from corda_amd import _lib
    key, kid, st, t = bytes(270), ctypes.c_uint32(), ctypes.c_uint8(), ctypes.c_uint64()
    b = _lib.KeyedSigBatch()
    assert lib.cordahip_vkey_add_rsa(None, key, 270, ctypes.byref(kid), ctypes.byref(st)) == -1
    assert lib.cordahip_vkey_add_rsa(None, None, 0, ctypes.byref(kid), ctypes.byref(st)) == -1
    assert lib.cordahip_rsa_verify_keyed(None, ctypes.byref(b)) == -1
    assert lib.cordahip_rsa_verify_keyed(None, None) == -1
    assert lib.cordahip_rsa_verify_keyed_submit(None, ctypes.byref(b), ctypes.byref(t)) == -1
    assert lib.cordahip_rsa_verify_keyed_submit(None, None, None) == -1
    assert lib.cordahip_rsa_verify_keyed_device(None, 0, None, None, None, None, 32, 96, 0, None, None, None) == -1
    assert lib.cordahip_rsa_public_op_keyed_device(None, 0, None, None, 96, 0, None, None) == -1
