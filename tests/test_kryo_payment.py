"""The two leaf kinds a payment adds (CORDAHIP_KRYO_MOVE_COMMAND = 18,
CORDAHIP_KRYO_SECURE_HASH = 19) on the CPU: cordahip_kryo_encode (host only) against the
Python model (tests/kryo_payment_model.py, built on oracle/kryo_leaves.py's Output /
OutputChunked / Graph), byte for byte, over both list forms, the hash present and absent,
1 / 2 / 3 / 12 / 13 signers, Ed25519 and SPKI keys and the four Move classes; the payloads
the header calls invalid are rejected, and every truncation of a valid payload is rejected
or encoded without a read outside it. PARITY UNPINNED: model and encoder restate the same
published rules, no JVM output confirms them."""
import ctypes
import itertools
import json
import os
import random

import numpy as np
import pytest

import kryo_payment_model as M
from corda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH = bytes(range(32))


def _keys(rng, n, sizes=(32,)):
    """n (class id, key bytes): Ed25519 (32 B, id 45) or SPKI (88 / 91 B, id 46)."""
    out = []
    for i in range(n):
        sz = sizes[i % len(sizes)]
        out.append((M.ED25519_CLASS if sz == 32 else M.SPKI_CLASS, bytes(rng.randrange(256) for _ in range(sz))))
    return out


def move_cases():
    """(class, keys, hash, array_list) over every shape the issue lists."""
    rng = random.Random(22)
    cases = []
    for al, h, n in itertools.product((True, False), (None, HASH), (1, 2, 3, 12, 13)):
        cases.append((M.CASH_MOVE, _keys(rng, n), h, al))
    for al, h, sizes in itertools.product((True, False), (None, HASH), ((88,), (91,), (32, 88, 91))):
        cases.append((M.CASH_MOVE, _keys(rng, len(sizes) + 1, sizes), h, al))
    for cls in M.MOVE_CLASSES:
        cases.append((cls, _keys(rng, 2), HASH, True))
        cases.append((cls, _keys(rng, 1), None, False))
    return cases


def move_item(case):
    cls, keys, h, al = case
    return ("move_command", _lib.pack_move_command(cls, keys, h, al), M.AAL_CLASS)


def _encode_raw(kind, payload, class_id=M.AAL_CLASS, cap=8192):
    """cordahip_kryo_encode of one item whose payload sits in a buffer of exactly its size: (rc, leaf)."""
    buf = np.frombuffer(bytes(payload) or b"\0", np.uint8).copy()
    it = _lib.KryoItem(_lib.KRYO_KINDS[kind], class_id, 0, buf.ctypes.data if payload else None, len(payload))
    off = np.zeros(2, np.uint64)
    out = np.zeros(cap, np.uint8)
    rc = _lib.lib().cordahip_kryo_encode(ctypes.byref(it), 1, out.ctypes.data, cap, off.ctypes.data)
    return rc, out[:int(off[1])].tobytes() if rc == 0 else b""


def test_golden_vectors_model_and_encoder():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "payment_leaf_vectors.json")))
    assert "parity unpinned" in g["status"] and "not by a JVM" in g["status"]
    assert [len(v["leaf"]) // 2 for v in g["vectors"]] == [199, 102, 334]
    for v in g["vectors"]:
        want = bytes.fromhex(v["leaf"])
        if v["kind"] == "secure_hash":
            assert M.secure_hash_leaf(bytes.fromhex(v["hash"])) == want
            assert _lib.kryo_encode([("secure_hash", bytes.fromhex(v["hash"]), 0)]) == [want]
            continue
        keys = [(kc, bytes.fromhex(k)) for kc, k in v["keys"]]
        h = bytes.fromhex(v["contract_hash"]) if v["contract_hash"] else None
        assert M.move_command_leaf(v["class"], keys, h, v["array_list"], v["aal_class"]) == want
        assert _lib.kryo_encode([("move_command", _lib.pack_move_command(v["class"], keys, h, v["array_list"]),
                                  v["aal_class"])]) == [want]


def test_move_leaf_lengths():
    """The issue's table: 1, 2 and 3 Ed25519 signers; 4 to 6 SHA-256 blocks."""
    k = [(M.ED25519_CLASS, HASH)] * 3
    table = {(True, False): [199, 233, 267], (True, True): [295, 329, 363],
             (False, False): [204, 238, 273], (False, True): [300, 334, 369]}
    for (al, has), want in table.items():
        got = _lib.kryo_encode([("move_command", _lib.pack_move_command(M.CASH_MOVE, k[:n], HASH if has else None, al),
                                 M.AAL_CLASS) for n in (1, 2, 3)])
        assert [len(x) for x in got] == want
        assert all(4 <= (len(x) + 9 + 63) // 64 <= 6 for x in got)


def test_move_command_equals_the_model_over_every_shape():
    cases = move_cases()
    got = _lib.kryo_encode([move_item(c) for c in cases])
    for (cls, keys, h, al), leaf in zip(cases, got):
        assert leaf == M.move_command_leaf(cls, keys, h, al), (cls, len(keys), h is not None, al, leaf.hex())
    # the class id is ignored for a java.util.ArrayList
    cls, keys, h, _ = cases[0]
    assert _encode_raw("move_command", _lib.pack_move_command(cls, keys, h, True), 7)[1] == got[0]
    assert _encode_raw("move_command", _lib.pack_move_command(cls, keys, h, False), 7)[1] == \
        M.move_command_leaf(cls, keys, h, False, aal_class=7)


def test_secure_hash_equals_the_model():
    rng = random.Random(5)
    hs = [HASH, bytes(32), b"\xff" * 32] + [bytes(rng.randrange(256) for _ in range(32)) for _ in range(5)]
    got = _lib.kryo_encode([("secure_hash", h, 0) for h in hs])
    for h, leaf in zip(hs, got):
        assert leaf == M.secure_hash_leaf(h) and len(leaf) == 102


def _head(name, keys):
    return _lib._pack_command_head(name, keys)


K1 = [(M.ED25519_CLASS, HASH)]
INVALID = {
    "name_len_0": bytes([0]) + bytes([1]) + _head("xx", K1)[4:] + b"\x00",
    "name_len_1": _head("M", K1) + b"\x00",
    "no_key": _head(M.CASH_MOVE, []) + b"\x00",
    "zero_length_key": _head(M.CASH_MOVE, [(M.ED25519_CLASS, b"")]) + b"\x00",
    "zero_length_second_key": _head(M.CASH_MOVE, K1 + [(M.ED25519_CLASS, b"")]) + b"\x02",
    "flags_4": _head(M.CASH_MOVE, K1) + b"\x04",
    "flags_80": _head(M.CASH_MOVE, K1) + b"\x81" + HASH,
    "no_flags": _head(M.CASH_MOVE, K1),
    "hash_flag_without_hash": _head(M.CASH_MOVE, K1) + b"\x01",
    "short_hash": _head(M.CASH_MOVE, K1) + b"\x01" + HASH[:31],
    "long_hash": _head(M.CASH_MOVE, K1) + b"\x01" + HASH + b"\x00",
    "hash_without_flag": _head(M.CASH_MOVE, K1) + b"\x02" + HASH,
    "trailing_byte": _head(M.CASH_MOVE, K1) + b"\x00\x00",
    "empty": b"",
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_move_payloads_are_rejected(name):
    assert _encode_raw("move_command", INVALID[name])[0] == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("n", [0, 31, 33])
def test_invalid_secure_hash_lengths_are_rejected(n):
    assert _encode_raw("secure_hash", bytes(n), 0)[0] == _lib.ERR_INVALID_ARG


def test_every_truncation_is_rejected_or_encoded():
    """Each cut of a valid payload in its own exact-size buffer (a read past it lands outside the
    payload); a Move payload has no valid proper prefix, so every cut is rejected."""
    rng = random.Random(9)
    for case in [(M.CASH_MOVE, _keys(rng, 3, (32, 88)), HASH, True), (M.MOVE_CLASSES[2], _keys(rng, 2), None, False)]:
        full = move_item(case)[1]
        assert _encode_raw("move_command", full)[1] == M.move_command_leaf(*case)
        for k in range(len(full)):
            assert _encode_raw("move_command", full[:k])[0] == _lib.ERR_INVALID_ARG, k
    for k in range(32):
        assert _encode_raw("secure_hash", HASH[:k], 0)[0] == _lib.ERR_INVALID_ARG


def test_pack_helpers_and_kinds():
    assert _lib.KRYO_KINDS["move_command"] == 18 and _lib.KRYO_KINDS["secure_hash"] == 19
    p = _lib.pack_move_command("ab", [(45, b"k")], HASH, False)
    assert p == b"\x02ab\x01\x2d\x00\x01\x00k\x01" + HASH
    assert _lib.pack_move_command("ab", [(45, b"k")])[-1] == _lib.MOVE_ARRAY_LIST
