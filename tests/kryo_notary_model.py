"""Python model of the two Kryo leaves a non-validating notary is shown
(NotaryFlow.kt:62: StateRef inputs and the TimeWindow), the checker of kinds
CORDAHIP_KRYO_STATE_REF / CORDAHIP_KRYO_TIME_WINDOW and of K21. TEST INFRASTRUCTURE
ONLY. Written with oracle/kryo_leaves.py's own Output / OutputChunked / Graph model
of Kryo 4.0.0's buffered writers, so the nested-flush framing is the one that file
states and the cash-issue kinds already use.

Rules (both classes are @CordaSerializable and unregistered: implicit NAME
registration, CompatibleFieldSerializer with EXTENDED field names in name order):
  StateRef(txhash: SecureHash, index: Int)              (Structures.kt:247)
    StateRef.index   primitive int: Output.writeInt(v, false) = zig-zag varint
    StateRef.txhash  declared SecureHash (not final): class SecureHash$SHA256 by
                     name, then OpaqueBytes.bytes (kryo_leaves.write_opaque)
  TimeWindow(fromTime: Instant?, untilTime: Instant?)   (Structures.kt:336-341)
    each side        java.time.Instant is final: NULL 00, or NOT_NULL 01 + body
    Instant body     TAKEN TO BE Kryo 4.0.0's TimeSerializers.InstantSerializer:
                     writeLong(epochSecond, true), writeInt(nano, true) -- plain
                     varints (a negative second: 9 bytes). Source: Kryo's published
                     source as recalled; that TimeSerializers is among 4.0.0's default
                     serializers is NOT checked here (no Kryo source, no JVM).
PARITY UNPINNED, like Party / the issue Command / the cash TransactionState: no
reference output confirms these bytes. tests/golden/notary_leaf_vectors.json holds
two vectors derived from these same rules.
"""
import hashlib

import kryo_leaves as K

STATE_REF = "net.corda.core.contracts.StateRef"
TIME_WINDOW = "net.corda.core.contracts.TimeWindow"
SHA256 = "net.corda.core.crypto.SecureHash$SHA256"
INSTANT_MIN_SECOND, INSTANT_MAX_SECOND = -31557014167219200, 31556889864403199
ABSENT = -(1 << 63)
SATURATE = 1 << 62

# every varint edge of a Java int's zig-zag form, and -1 as its u32 image
INDEX_EDGES = [0, 1, 63, 64, 8191, 8192, 2**20 - 1, 2**20, 2**27 - 1, 2**27, 2**31 - 1, 0xFFFFFFFF]
SECOND_EDGES = [0, 127, 128, 2**34, -1, INSTANT_MIN_SECOND, INSTANT_MAX_SECOND]
NANO_EDGES = [0, 127, 128, 999999999]


def java_int(index: int) -> int:
    """A cordahip_state_ref's u32 index as the Java int it stands for."""
    index &= 0xFFFFFFFF
    return index - (1 << 32) if index >> 31 else index


def varlong(v: int) -> bytes:
    """Output.writeVarLong(v, true): 7-bit groups, low first; the 9th byte takes 8 bits."""
    v &= (1 << 64) - 1
    out = bytearray()
    for _ in range(8):
        if v >> 7 == 0:
            out.append(v)
            return bytes(out)
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def state_ref_leaf(txhash: bytes, index: int) -> bytes:
    assert len(txhash) == 32

    def write(out, g):
        g.write_class_name(out, STATE_REF)
        g.compatible_fields(out, STATE_REF, [
            ("StateRef.index", lambda o: o.write_atomic(K.varint_zigzag(java_int(index)))),
            ("StateRef.txhash", lambda o: K.write_opaque(o, g, SHA256, bytes(txhash)))])

    return K._leaf(write)


def window_valid(from_time, until_time) -> bool:
    return all(side is None or (0 <= side[1] <= 999999999 and INSTANT_MIN_SECOND <= side[0] <= INSTANT_MAX_SECOND)
               for side in (from_time, until_time))


def time_window_leaf(from_time, until_time) -> bytes:
    """A side is None or (epochSecond, nano); both None is encoded (two NULL markers)."""
    if not window_valid(from_time, until_time):
        raise ValueError("not an Instant")

    def side(o, t):
        if t is None:
            o.write(0)  # NULL
            return
        o.write(1)  # NOT_NULL
        o.write_atomic(varlong(t[0]))
        o.write_atomic(K.varint(t[1]))

    def write(out, g):
        g.write_class_name(out, TIME_WINDOW)
        g.compatible_fields(out, TIME_WINDOW, [("TimeWindow.fromTime", lambda o: side(o, from_time)),
                                               ("TimeWindow.untilTime", lambda o: side(o, until_time))])

    return K._leaf(write)


def instant_ns(t) -> int:
    """cordahip_commit_batch's form of a window side: ns since the epoch, saturated at +-2^62."""
    if t is None:
        return ABSENT
    return max(-SATURATE, min(SATURATE, t[0] * 10**9 + t[1]))


def sha256(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def edge_refs():
    """(txhash, index) over INDEX_EDGES, the hashes distinct and fixed."""
    return [(sha256(b"ref %d" % i), ix) for i, ix in enumerate(INDEX_EDGES)]


def edge_windows():
    """Valid windows over SECOND_EDGES x NANO_EDGES on either side, and all four flags values."""
    ws = [(None, None), ((0, 0), None), (None, (0, 0)), ((1500000000, 5), (1500000030, 0))]
    for s in SECOND_EDGES:
        for n in NANO_EDGES:
            ws.append(((s, n), None))
            ws.append((None, (s, n)))
            ws.append(((s, n), (SECOND_EDGES[(SECOND_EDGES.index(s) + 1) % len(SECOND_EDGES)], n)))
    return ws
