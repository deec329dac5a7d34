"""The RSA routing and signed-transaction RSA switches at the drop-in boundary (CPU-only): the three
new functions are declared in include/cordahip.h with the argument lists the ctypes bindings use,
are exported by the library, leave the ABI version at 4, and answer CORDAHIP_ERR_INVALID_ARG
without a context or without output pointers; the scratch layout is the one the header documents."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NEW = {"cordahip_vkey_set_routing_rsa": 2, "cordahip_vkey_route_stats_rsa": 4, "cordahip_set_rsa_on_device": 2}


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
    # the argument types, as the header spells them
    assert re.search(r"cordahip_vkey_set_routing_rsa\s*\(\s*cordahip_ctx\s*\*\s*ctx,\s*uint32_t\s+on\s*\)", src)
    assert re.search(r"cordahip_set_rsa_on_device\s*\(\s*cordahip_ctx\s*\*\s*ctx,\s*uint32_t\s+on\s*\)", src)
    assert re.search(r"cordahip_vkey_route_stats_rsa\s*\(\s*cordahip_ctx\s*\*\s*ctx,\s*int\s+device,\s*uint64_t\s*\*\s*"
                     r"keyed_rows,\s*uint64_t\s*\*\s*generic_rows\s*\)", src)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    assert lib.cordahip_vkey_route_stats_rsa.argtypes == [ctypes.c_void_p, ctypes.c_int32, u64p, u64p]
    assert lib.cordahip_vkey_set_routing_rsa.argtypes == [ctypes.c_void_p, ctypes.c_uint32]
    assert lib.cordahip_set_rsa_on_device.argtypes == [ctypes.c_void_p, ctypes.c_uint32]


def test_null_context_or_outputs_is_invalid_arg(lib):
    k, g = ctypes.c_uint64(), ctypes.c_uint64()
    assert lib.cordahip_vkey_set_routing_rsa(None, 1) == -1
    assert lib.cordahip_vkey_set_routing_rsa(None, 0) == -1
    assert lib.cordahip_set_rsa_on_device(None, 1) == -1
    assert lib.cordahip_set_rsa_on_device(None, 0) == -1
    assert lib.cordahip_vkey_route_stats_rsa(None, 0, ctypes.byref(k), ctypes.byref(g)) == -1
    assert lib.cordahip_vkey_route_stats_rsa(None, 0, None, None) == -1
    assert lib.cordahip_vkey_route_stats_rsa(None, 0, ctypes.byref(k), None) == -1
    assert lib.cordahip_vkey_route_stats_rsa(None, 0, None, ctypes.byref(g)) == -1


def test_scratch_layout_matches_header_text():
    hpp = open(os.path.join(ROOT, "corda_amd", "csrc", "rsa_route.hpp")).read()
    assert "kRsaRouteHdrWords = 16" in hpp and "return kRsaRouteHdrWords + 3 * cap;" in hpp
    doc = open(HEADER).read()
    assert re.search(r"64 bytes and 12 bytes per row", doc)
    assert "CORDAHIP_RSA_WS_ROWS" in doc
