"""The two leaf kinds a notary tear-off is made of (CORDAHIP_KRYO_STATE_REF = 16,
CORDAHIP_KRYO_TIME_WINDOW = 17) on the CPU: cordahip_kryo_encode (host only) against the
Python model (tests/kryo_notary_model.py, built on oracle/kryo_leaves.py's Output /
OutputChunked / Graph), byte for byte, at every varint edge; the rows the header calls
invalid are rejected; the counting mode gives the encoded size. PARITY UNPINNED: model
and encoder restate the same published rules, no JVM output confirms them (the Instant
body in particular is Kryo 4.0.0's TimeSerializers.InstantSerializer as recalled)."""
import ctypes
import json
import os

import numpy as np
import pytest

import kryo_notary_model as M
from corda_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _encode_raw(kind, payload, cap):
    """cordahip_kryo_encode of one item with an explicit payload and capacity: (rc, leaf, size)."""
    buf = np.frombuffer(bytes(payload) or b"\0", np.uint8).copy()
    it = _lib.KryoItem(_lib.KRYO_KINDS[kind], 0, 0, buf.ctypes.data, len(payload))
    off = np.zeros(2, np.uint64)
    out = np.zeros(max(cap, 1), np.uint8)
    rc = _lib.lib().cordahip_kryo_encode(ctypes.byref(it), 1, out.ctypes.data, cap, off.ctypes.data)
    return rc, out[:int(off[1])].tobytes() if rc == 0 else b"", int(off[1])


def test_golden_vectors_model_and_encoder():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "notary_leaf_vectors.json")))
    assert "parity unpinned" in g["status"]
    sr, tw = g["vectors"]
    want = bytes.fromhex(sr["leaf"])
    assert len(want) == 173
    assert M.state_ref_leaf(bytes.fromhex(sr["txhash"]), sr["index"]) == want
    assert _lib.kryo_encode([("state_ref", _lib.pack_state_ref(bytes.fromhex(sr["txhash"]), sr["index"]), 0)]) == [want]
    want = bytes.fromhex(tw["leaf"])
    f, u = tuple(tw["from"]), tuple(tw["until"])
    assert M.time_window_leaf(f, u) == want
    assert _lib.kryo_encode([("time_window", _lib.pack_time_window(f, u), 0)]) == [want]


def test_state_ref_at_every_varint_edge():
    refs = M.edge_refs()
    got = _lib.kryo_encode([("state_ref", _lib.pack_state_ref(h, ix), 0) for h, ix in refs])
    sizes = set()
    for (h, ix), leaf in zip(refs, got):
        assert leaf == M.state_ref_leaf(h, ix), (ix, leaf.hex())
        assert (len(leaf) + 9 + 63) // 64 == 3  # always 3 SHA-256 blocks
        sizes.add(len(leaf))
    assert sizes == {173, 174, 175, 176, 177}
    # -1 and its u32 image are one Java int
    assert M.state_ref_leaf(refs[0][0], -1) == M.state_ref_leaf(refs[0][0], 0xFFFFFFFF)


def test_time_window_at_every_edge_and_all_flags():
    ws = M.edge_windows()
    assert {(f is not None) | ((u is not None) << 1) for f, u in ws} == {0, 1, 2, 3}
    got = _lib.kryo_encode([("time_window", _lib.pack_time_window(f, u), 0) for f, u in ws])
    for (f, u), leaf in zip(ws, got):
        assert leaf == M.time_window_leaf(f, u), (f, u, leaf.hex())
        # 85 bytes of header, names and field names; a side is 3 bytes (NULL) .. 17 (a negative
        # second in 9 bytes, a nano of 2^28 or more in 5): 91..119, always 2 SHA-256 blocks
        assert 91 <= len(leaf) <= 119 and (len(leaf) + 9 + 63) // 64 == 2
    lens = {len(x) for x in got}
    assert 91 in lens and 119 in lens
    # a negative second takes 9 bytes (plain varlong, not zig-zag)
    assert len(M.time_window_leaf((-1, 0), None)) - len(M.time_window_leaf((0, 0), None)) == 8


@pytest.mark.parametrize("payload", [
    _lib.pack_state_ref(bytes(32), 0)[:35], _lib.pack_state_ref(bytes(32), 0) + b"\0", b"",
], ids=["short", "long", "empty"])
def test_invalid_state_ref_rows_are_rejected(payload):
    rc, _, _ = _encode_raw("state_ref", payload, 4096)
    assert rc == _lib.ERR_INVALID_ARG


def _tw(flags, fs=0, fn=0, us=0, un=0):
    return (bytes([flags]) + int(fs).to_bytes(8, "little", signed=True) + int(fn).to_bytes(4, "little", signed=True)
            + int(us).to_bytes(8, "little", signed=True) + int(un).to_bytes(4, "little", signed=True))


INVALID_WINDOWS = {
    "short": _tw(3)[:24], "long": _tw(3) + b"\0", "empty": b"",
    "flags4": _tw(4), "flags80": _tw(0x83), "flagsff": _tw(0xFF),
    "from_nano_neg": _tw(1, 0, -1), "from_nano_big": _tw(1, 0, 1000000000),
    "until_nano_neg": _tw(2, 0, 0, 0, -1), "until_nano_big": _tw(2, 0, 0, 0, 1000000000),
    "from_s_low": _tw(1, M.INSTANT_MIN_SECOND - 1), "from_s_high": _tw(1, M.INSTANT_MAX_SECOND + 1),
    "until_s_low": _tw(2, 0, 0, M.INSTANT_MIN_SECOND - 1), "until_s_high": _tw(3, 0, 0, M.INSTANT_MAX_SECOND + 1),
}


@pytest.mark.parametrize("name", sorted(INVALID_WINDOWS))
def test_invalid_window_rows_are_rejected(name):
    rc, _, _ = _encode_raw("time_window", INVALID_WINDOWS[name], 4096)
    assert rc == _lib.ERR_INVALID_ARG


def test_absent_side_ignores_its_fields():
    """Only a present side is validated and written: garbage behind an absent one changes nothing."""
    rc, leaf, _ = _encode_raw("time_window", _tw(1, 5, 6, 2**62, -7), 4096)
    assert rc == 0 and leaf == M.time_window_leaf((5, 6), None)
    rc, leaf, _ = _encode_raw("time_window", _tw(0, 2**62, -1, -2**62, 2**31 - 1), 4096)
    assert rc == 0 and leaf == M.time_window_leaf(None, None)


def test_counting_mode_gives_the_size():
    for kind, payload, want in [
            ("state_ref", _lib.pack_state_ref(bytes(range(32)), 2**27), None),
            ("time_window", _lib.pack_time_window((-1, 999999999), (2**34, 128)), None)]:
        rc, leaf, size = _encode_raw(kind, payload, 4096)
        assert rc == 0 and size == len(leaf)
        rc0, _, need = _encode_raw(kind, payload, 0)  # no room: the size comes back, nothing is written
        assert rc0 == _lib.ERR_BUFFER_TOO_SMALL and need == size


def test_instant_ns_reference():
    assert M.instant_ns(None) == M.ABSENT
    assert M.instant_ns((4611686018, 427387903)) == 2**62 - 1
    assert M.instant_ns((4611686018, 427387904)) == 2**62
    assert M.instant_ns((4611686018, 427387905)) == 2**62
    assert M.instant_ns((-4611686019, 572612096)) == -2**62
    assert M.instant_ns((-4611686019, 572612095)) == -2**62
    assert M.instant_ns((M.INSTANT_MAX_SECOND, 0)) == 2**62 and M.instant_ns((M.INSTANT_MIN_SECOND, 0)) == -2**62
