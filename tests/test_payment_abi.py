"""K22's additions to the ABI are additive: the header defines kinds 18 and 19 and declares
cordahip_txcomp_inputs_device, corda_amd._lib binds it, and CORDAHIP_ABI_VERSION is still 4."""
import os
import re

from corda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "cordahip.h")).read()


def test_header_defines_the_kinds_and_the_call():
    assert re.search(r"^#define CORDAHIP_KRYO_MOVE_COMMAND 18$", HEADER, re.M)
    assert re.search(r"^#define CORDAHIP_KRYO_SECURE_HASH 19$", HEADER, re.M)
    m = re.search(r"^int cordahip_txcomp_inputs_device\(([^;]*)\);", HEADER, re.M)
    assert m
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert len(args) == 16
    assert re.search(r"^#define CORDAHIP_ABI_VERSION 4u$", HEADER, re.M)
    # both kinds say what they are not: checked against a JVM
    block = HEADER[HEADER.index("MOVE_COMMAND   net.corda"):HEADER.index("#define CORDAHIP_KRYO_MOVE_COMMAND")]
    assert "PARITY UNPINNED" in block


def test_lib_binds_the_call_and_the_kinds():
    assert "cordahip_txcomp_inputs_device" in _lib.EXPORTS
    assert _lib.KRYO_KINDS["move_command"] == 18 and _lib.KRYO_KINDS["secure_hash"] == 19
    assert _lib.ABI_VERSION == 4
    lib = _lib.lib()
    assert lib.cordahip_abi_version() == 4
    f = lib.cordahip_txcomp_inputs_device
    assert len(f.argtypes) == 16
    # INVALID_ARG before anything is touched: a NULL context
    assert f(None, 0, None, 0, None, 0, None, 0, None, None, 0, None, None, None, None, None) == _lib.ERR_INVALID_ARG
