"""The RSA signing entry points at the drop-in boundary (CPU-only), as
tests/test_ecdsa_sign_abi.py does for the ECDSA signer: cordahip_rsa_private_key and
cordahip_rsa_sign_batch as ctypes lays them out against the C compiler's layout of
include/cordahip.h, the constants against the header, status.hpp, rsa_sign.hpp and the Python
mirror, the table size the header documents, and every new entry point answering
CORDAHIP_ERR_INVALID_ARG without a context. (Bad offsets and a NULL salt with outputs
untouched need a context: tests/test_gpu_rsa_sign.py; the CSR check is check_sign_batch, the
other signing calls', fuzzed on the host by tests/test_ecdsa_sign_csr_fuzz.py.)"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cordahip.h")
NEW = ["cordahip_signer_add_rsa", "cordahip_rsa_sign", "cordahip_rsa_sign_submit", "cordahip_rsa_sign_keyed_device"]


@pytest.fixture(scope="module")
def lib():
    from corda_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "corda_amd", "csrc")])
    return _lib.lib()


def test_struct_layouts_match_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc absent")
    from corda_amd import _lib
    structs = [(_lib.RsaPrivateKey, "cordahip_rsa_private_key", 64,
                ["p", "q", "dp", "dq", "qinv", "p_len", "q_len", "dp_len", "dq_len", "qinv_len", "e"]),
               (_lib.RsaSignBatch, "cordahip_rsa_sign_batch", 80,
                ["n", "key_id", "msg", "msg_off", "gate", "salt", "sig", "sig_len", "status", "msg_bytes"])]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cordahip.h"', "int main(void) {",
             'printf("CORDAHIP_SIGN_FAILED %d\\n", (int)CORDAHIP_SIGN_FAILED);',
             'printf("CORDAHIP_RSA_SIGNER_MAX_KEYS %d\\n", (int)CORDAHIP_RSA_SIGNER_MAX_KEYS);',
             'printf("CORDAHIP_RSA_SIG_SLOT %d\\n", (int)CORDAHIP_RSA_SIG_SLOT);']
    for cls, cname, _, fields in structs:
        assert [f[0] for f in cls._fields_] == fields
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    for cls, cname, size, fields in structs:
        assert int(got[cname]) == ctypes.sizeof(cls) == size
        for f in fields:
            assert int(got["%s.%s" % (cname, f)]) == getattr(cls, f).offset, (cname, f)
    assert int(got["CORDAHIP_SIGN_FAILED"]) == _lib.SIGN_FAILED == 16
    assert int(got["CORDAHIP_RSA_SIGNER_MAX_KEYS"]) == _lib.RSA_SIGNER_MAX_KEYS == 64
    assert int(got["CORDAHIP_RSA_SIG_SLOT"]) == _lib.RSA_SIG_SLOT == 512


def test_constants_match_header_and_sources():
    from corda_amd import _lib
    src = open(HEADER).read()
    assert "#define CORDAHIP_ABI_VERSION 4u" in src  # additive
    assert "#define CORDAHIP_RSA_SIGNER_MAX_KEYS 64" in src and "#define CORDAHIP_RSA_SIG_SLOT 512" in src
    assert re.search(r"enum \{ CORDAHIP_SIGN_FAILED = 16 \};", src)
    st = open(os.path.join(ROOT, "corda_amd", "csrc", "status.hpp")).read()
    assert re.search(r"kSignFailed = 16;", st) and re.search(r"kSignUnknownKey = 14;", st)
    core = open(os.path.join(ROOT, "corda_amd", "csrc", "rsa_sign.hpp")).read()
    assert re.search(r"kSignerMaxKeys = 64;", core) and "#define CORDAHIP_RSA_SIGN_WIN 3" in core
    assert re.search(r"kSignSlots = 4096;", core)
    # the table the header describes: the index over the pool's slots, 64 records of 840 words, the scratch
    rec_words = 8 + 3 * 128 + 7 * 64
    scratch = 4 + 128 + 4 + 128 + 2 + 2
    assert rec_words * 4 == 3360 and "3360 bytes" in src
    assert (4096 + 64 * rec_words + scratch) * 4 == _lib.RSA_SIGN_TABLE_BYTES == 232496 < 512 * 1024
    assert "232,496 bytes" in src and "kSignTabBytes == 232496" in core
    # the header no longer says RSA signing is not offered
    assert "RSA signing and CompositeSignature assembly are not" not in src
    assert "PARITY UNPINNED" in src[src.index("RSA_SHA256 batch signing"):src.index("CORDAHIP_RSA_SIGNER_MAX_KEYS 64")]


def test_new_entry_points_declared_and_exported(lib):
    from corda_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for f in NEW:
        assert re.search(r"\b%s\s*\(" % f, src), f
        assert f in _lib.EXPORTS and getattr(lib, f) is not None, f


def test_null_context_is_invalid_arg(lib):
    from corda_amd import _lib
    one = b"\x05"
    key = _lib.RsaPrivateKey(one, one, one, one, one, 1, 1, 1, 1, 1, 3)
    kid, st, ml, t = ctypes.c_uint32(), ctypes.c_uint8(), ctypes.c_uint32(), ctypes.c_uint64()
    mod = ctypes.create_string_buffer(512)
    b = _lib.RsaSignBatch()
    assert lib.cordahip_signer_add_rsa(None, ctypes.byref(key), ctypes.byref(kid), ctypes.byref(st), mod,
                                       ctypes.byref(ml)) == -1
    assert lib.cordahip_signer_add_rsa(None, None, None, None, None, None) == -1
    assert lib.cordahip_rsa_sign(None, ctypes.byref(b)) == -1
    assert lib.cordahip_rsa_sign(None, None) == -1
    assert lib.cordahip_rsa_sign_submit(None, ctypes.byref(b), ctypes.byref(t)) == -1
    assert lib.cordahip_rsa_sign_submit(None, None, None) == -1
    assert lib.cordahip_rsa_sign_keyed_device(None, 0, None, None, 32, None, 64, 0, None, None, None, None,
                                              None) == -1


def test_engine_mirror_has_the_calls():
    from corda_amd import engine, resolve
    for name in ("signer_add_rsa", "rsa_sign_batch", "rsa_sign_keyed_device", "signer_family"):
        assert callable(getattr(engine.Engine, name)), name
    assert callable(resolve._sign_with)


def test_sign_with_takes_the_rsa_branch():
    """resolve._sign_with hands an RSA signer id to Engine.rsa_sign_batch with the caller's salts,
    or with 32 fresh bytes a lane; the other families go where they went"""
    import numpy as np
    from corda_amd import resolve

    class Fake:
        def __init__(self):
            self.calls = []

        def signer_family(self, k):
            return {1: "rsa", 2: "ed25519", 3: 3}.get(k)

        def rsa_sign_batch(self, ids, msgs, salts, gate=None):
            self.calls.append(("rsa", list(salts)))
            rows = np.zeros((len(msgs), 512), np.uint8)
            rows[:, :3] = 7
            return rows, np.full(len(msgs), 3, np.uint16), np.zeros(len(msgs), np.uint8)

        def sign_batch(self, ids, msgs, gate=None):
            self.calls.append(("ed",))
            return np.zeros((len(msgs), 64), np.uint8), np.zeros(len(msgs), np.uint8)

        def ecdsa_sign_batch(self, ids, msgs, gate=None):
            self.calls.append(("ec",))
            return np.zeros((len(msgs), 72), np.uint8), np.full(len(msgs), 8, np.uint8), np.zeros(len(msgs), np.uint8)

    f = Fake()
    msgs = [b"a" * 32, b"b" * 32]
    sigs, _ = resolve._sign_with(f, 1, msgs, None, salts=[b"s" * 32, b"t" * 32])
    assert sigs == [b"\x07" * 3] * 2 and f.calls[-1] == ("rsa", [b"s" * 32, b"t" * 32])
    resolve._sign_with(f, 1, msgs, None)
    drawn = f.calls[-1][1]
    assert len(drawn) == 2 and all(len(s) == 32 for s in drawn) and drawn[0] != drawn[1]
    assert [len(s) for s in resolve._sign_with(f, 2, msgs, None)[0]] == [64, 64] and f.calls[-1] == ("ed",)
    assert [len(s) for s in resolve._sign_with(f, 3, msgs, None)[0]] == [8, 8] and f.calls[-1] == ("ec",)
