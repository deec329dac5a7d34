"""The switch of routing inside the mixed device-resident calls (K24) at the drop-in boundary
(CPU-only): cordahip_vkey_set_routing_device is declared in include/cordahip.h with the argument
list the ctypes binding uses, is exported by the library, leaves the ABI version at 4, answers
CORDAHIP_ERR_INVALID_ARG without a context, and the header documents its default and says at both
mixed calls that registered keys are consulted when it is on."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NAME = "cordahip_vkey_set_routing_device"


@pytest.fixture(scope="module")
def lib():
    from corda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "corda_amd", "csrc")])
    return _lib.lib()


def test_switch_declared_bound_and_exported(lib):
    from corda_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "#define CORDAHIP_ABI_VERSION 4u" in src and _lib.ABI_VERSION == 4
    assert lib.cordahip_abi_version() == 4
    assert re.search(r"\bint\s+%s\s*\(\s*cordahip_ctx\s*\*\s*ctx,\s*uint32_t\s+on\s*\)\s*;" % NAME, src)
    assert NAME in _lib.EXPORTS
    f = getattr(lib, NAME)
    assert f.argtypes == [ctypes.c_void_p, ctypes.c_uint32]
    assert f.restype is ctypes.c_int32 or f.restype is ctypes.c_int
    from corda_amd.engine import Engine
    assert callable(getattr(Engine, "vkey_set_routing_device"))


def test_null_context_is_invalid_arg(lib):
    assert getattr(lib, NAME)(None, 1) == -1
    assert getattr(lib, NAME)(None, 0) == -1


def test_header_documents_default_and_both_mixed_calls():
    doc = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    sec = doc[doc.index("Routing inside the mixed device-resident calls (K24)"):]
    sec = sec[:sec.index("int %s" % NAME)]
    assert "0 (the default) off" in sec
    assert "nothing more is launched, allocated or locked" in sec and "no route counter moves" in sec
    for fam in ("cordahip_vkey_set_routing (Ed25519)", "cordahip_vkey_set_routing_ecdsa",
                "cordahip_vkey_set_routing_rsa"):
        assert fam in sec, fam
    # the sentence at cordahip_sig_verify_device and at the signed-tx device calls
    assert len(re.findall(r"[Rr]egistered keys are not consulted[^.]*unless cordahip_vkey_set_routing_device is on",
                          doc)) == 2
