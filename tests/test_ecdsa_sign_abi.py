"""The ECDSA signing entry points at the drop-in boundary (CPU-only), as
tests/test_sign_abi.py does for the Ed25519 signer: cordahip_ecdsa_sign_batch as ctypes
lays it out against the C compiler's layout of include/cordahip.h, CORDAHIP_SIGN_FAILED
against the header, status.hpp and the Python mirror, the table layout the header
documents, and every new entry point answering CORDAHIP_ERR_INVALID_ARG without a
context. (Bad offsets with outputs untouched need a context: tests/test_gpu_ecdsa_sign.py;
the check itself is fuzzed on the host by tests/test_ecdsa_sign_csr_fuzz.py.)"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NEW = ["cordahip_signer_add_ecdsa", "cordahip_ecdsa_sign", "cordahip_ecdsa_sign_submit",
       "cordahip_ecdsa_sign_keyed_device"]


@pytest.fixture(scope="module")
def lib():
    from corda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "corda_amd", "csrc")])
    return _lib.lib()


def test_ecdsa_sign_batch_layout_matches_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc absent")
    from corda_amd import _lib
    cls, cname = _lib.EcdsaSignBatch, "cordahip_ecdsa_sign_batch"
    assert [f[0] for f in cls._fields_] == ["n", "key_id", "msg", "msg_off", "gate", "sig", "sig_len", "status",
                                            "msg_bytes"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cordahip.h"', "int main(void) {",
             'printf("CORDAHIP_SIGN_FAILED %d\\n", (int)CORDAHIP_SIGN_FAILED);',
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f in cls._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f[0], cname, f[0]))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls) == 72
    assert int(got["CORDAHIP_SIGN_FAILED"]) == _lib.SIGN_FAILED == 16
    for f in cls._fields_:
        assert int(got["%s.%s" % (cname, f[0])]) == getattr(cls, f[0]).offset, f[0]


def test_sign_failed_status_matches_header():
    from corda_amd import _lib
    src = open(HEADER).read()
    # an enumerator (the header says why); the C compiler's value of it is checked below
    assert re.search(r"enum \{ CORDAHIP_SIGN_FAILED = 16 \};", src) and _lib.SIGN_FAILED == 16
    assert "#define CORDAHIP_ABI_VERSION 4u" in src
    # no generic lane status has the value (a keyed verifier's UNKNOWN_KEY is another call's)
    others = [int(v) for v in re.findall(r"#define CORDAHIP_STATUS_\w+ (\d+)", src)]
    assert 16 not in others and not {_lib.SIGN_UNKNOWN_KEY, _lib.SIGN_SKIPPED} & {16}
    st = open(os.path.join(ROOT, "corda_amd", "csrc", "status.hpp")).read()
    assert re.search(r"kSignFailed = 16;", st)
    core = open(os.path.join(ROOT, "corda_amd", "csrc", "ecdsa_sign_core.hpp")).read()
    # the bound, the slot and the probability the header states for it
    assert re.search(r"kEcSignMaxTries = 8;", core) and re.search(r"kEcSignSigBytes = 72;", core)
    assert _lib.ECDSA_SIG_SLOT == 72 and "bounded at 8 candidates" in src and "below 2^-250" in src
    # the table the header describes: two 40 KiB comb tables, 4096 records of 128 bytes, the scratch
    words = 2 * 64 * 8 * 20 + 4096 * 32 + 8 + 20
    assert words * 4 == 606320 and "592 KB per" in src and 606320 // 1024 == 592


def test_new_entry_points_declared_and_exported(lib):
    from corda_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, src), f
        assert f in _lib.EXPORTS and getattr(lib, f) is not None, f


def test_null_context_is_invalid_arg(lib):
    from corda_amd import _lib
    d, pub, kid, st, t = bytes(31) + b"\x01", ctypes.create_string_buffer(65), ctypes.c_uint32(), ctypes.c_uint8(), \
        ctypes.c_uint64()
    b = _lib.EcdsaSignBatch()
    assert lib.cordahip_signer_add_ecdsa(None, 3, d, ctypes.byref(kid), ctypes.byref(st), pub) == -1
    assert lib.cordahip_ecdsa_sign(None, ctypes.byref(b)) == -1
    assert lib.cordahip_ecdsa_sign(None, None) == -1
    assert lib.cordahip_ecdsa_sign_submit(None, ctypes.byref(b), ctypes.byref(t)) == -1
    assert lib.cordahip_ecdsa_sign_submit(None, None, None) == -1
    assert lib.cordahip_ecdsa_sign_keyed_device(None, 0, None, None, 32, 0, None, None, None, None, None) == -1


def test_engine_mirror_has_the_calls():
    from corda_amd import engine, resolve
    for name in ("signer_add_ecdsa", "ecdsa_sign_batch", "ecdsa_sign_keyed_device", "signer_family"):
        assert callable(getattr(engine.Engine, name)), name
    assert callable(resolve._sign_with)
