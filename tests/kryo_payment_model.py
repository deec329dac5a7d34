"""Python model of what a payment adds to a cash issue (K22): the Kryo leaves of kinds
CORDAHIP_KRYO_MOVE_COMMAND / CORDAHIP_KRYO_SECURE_HASH, and the rule by which
cordahip_txcomp_inputs_device takes a component batch's inputs and windows out of its
items. TEST INFRASTRUCTURE ONLY. The leaves are written with oracle/kryo_leaves.py's own
Output / OutputChunked / Graph model of Kryo 4.0.0's buffered writers, as
tests/kryo_notary_model.py is.

Rules (every class is @CordaSerializable and unregistered unless said otherwise: implicit
NAME registration, CompatibleFieldSerializer with EXTENDED field names in name order):
  Command(value, signers)                                   (Structures.kt:285)
    Command.signers  java.util.Arrays$ArrayList (TransactionBuilder.addCommand): registered,
                     ArraysAsListSerializer -- class id, length, component class
                     java.security.PublicKey by name, the elements (kryo_leaves'
                     write_issue_command); or java.util.ArrayList (OnLedgerAsset.generateSpend,
                     OnLedgerAsset.kt:93,121: gathered.map { }): unregistered, by name,
                     Kryo's CollectionSerializer -- varint(size), class and object per
                     element (as Cash.State.exitKeys' LinkedHashSet)
    Command.value    the Move class by name (Cash.kt:142, CommodityContract.kt:125,
                     Obligation.kt:348, CommercialPaper.kt:190), its one field
                     "<Simple>.contractHash", declared SecureHash? (not final): null is
                     writeClass(null) = 00; else SecureHash$SHA256 by name + OpaqueBytes.bytes
  SecureHash$SHA256 as a component (an attachment id): by name (id 0), OpaqueBytes.bytes
PARITY UNPINNED, like every composite kind: no reference output confirms these bytes.
tests/golden/payment_leaf_vectors.json holds three vectors derived from these same rules.
"""
import kryo_leaves as K
import kryo_notary_model as N

COMMAND = "net.corda.core.contracts.Command"
SHA256 = N.SHA256
MOVE_CLASSES = [
    "net.corda.contracts.asset.Cash$Commands$Move",
    "net.corda.contracts.asset.CommodityContract$Commands$Move",
    "net.corda.contracts.asset.Obligation$Commands$Move",
    "net.corda.contracts.CommercialPaper$Commands$Move",
]
CASH_MOVE = MOVE_CLASSES[0]
ED25519_CLASS, AAL_CLASS, SPKI_CLASS = 45, 61, 46  # registration ids as the tests use them
TX_BAD_COMPONENT = 9
KIND_STATE_REF, KIND_TIME_WINDOW = 16, 17


def move_command_leaf(cls, keys, contract_hash=None, array_list=True, aal_class=AAL_CLASS) -> bytes:
    """keys: [(key class id, key bytes)]; contract_hash: None or 32 bytes."""
    assert keys and (contract_hash is None or len(contract_hash) == 32)

    def write(out, g):
        def signers(o):
            if array_list:
                g.write_class_name(o, "java.util.ArrayList")
                o.write_atomic(K.varint(len(keys)))
            else:
                K.Graph.write_class_id(o, aal_class)
                o.write_atomic(K.varint(len(keys)))
                g.write_class_name(o, "java.security.PublicKey")
            for kc, k in keys:
                K.write_key(o, kc, bytes(k))

        simple = cls.replace("$", ".").rsplit(".", 1)[-1]

        def contract_hash_field(c):
            if contract_hash is None:
                c.write_atomic(K.varint(0))  # writeClass(null)
            else:
                K.write_opaque(c, g, SHA256, bytes(contract_hash))

        def value(o):
            g.write_class_name(o, cls)
            g.compatible_fields(o, cls, [(simple + ".contractHash", contract_hash_field)])

        g.write_class_name(out, COMMAND)
        g.compatible_fields(out, COMMAND, [("Command.signers", signers), ("Command.value", value)])

    return K._leaf(write)


def secure_hash_leaf(h: bytes) -> bytes:
    assert len(h) == 32
    return K._leaf(lambda out, g: K.write_opaque(out, g, SHA256, bytes(h)))


def unpack_move_command(p: bytes):
    """A valid MOVE_COMMAND payload -> (class name, keys, contract hash or None, array_list)."""
    n = p[0]
    cls, nkeys, at, keys = p[1:1 + n].decode("ascii"), p[1 + n], 2 + n, []
    for _ in range(nkeys):
        kc, kl = int.from_bytes(p[at:at + 2], "little"), int.from_bytes(p[at + 2:at + 4], "little")
        keys.append((kc, p[at + 4:at + 4 + kl]))
        at += 4 + kl
    flags = p[at]
    assert not flags & ~3 and len(p) == at + 1 + (32 if flags & 1 else 0)
    return cls, keys, (p[at + 1:] if flags & 1 else None), bool(flags & 2)


def component_leaf(kind, value, class_id) -> bytes:
    """The model's leaf of one component in _lib.kryo_pack's (kind, value, class_id) form: the
    payment kinds and the notary's two from the models, every other kind from oracle/kryo_leaves.py."""
    if kind == "state_ref":
        return N.state_ref_leaf(value[:32], int.from_bytes(value[32:], "little"))
    if kind == "time_window":
        return N.time_window_leaf(*_window(value))
    if kind == "move_command":
        cls, keys, h, al = unpack_move_command(bytes(value))
        return move_command_leaf(cls, keys, h, al, class_id)
    if kind == "secure_hash":
        return secure_hash_leaf(bytes(value))
    return K.leaf(kind, value, class_id)


# ---- the extraction rule (cordahip_txcomp_inputs_device) ---------------------------------
def _payload(payload, off, length, want):
    """The item's payload, or None when it is not `want` bytes wholly inside `payload`."""
    if length != want or off > len(payload) or want > len(payload) - off:
        return None
    return bytes(payload[off:off + want])


def _window(row):
    """A 25-byte TIME_WINDOW row -> (from, until) sides as N.time_window_leaf takes them, or None if invalid."""
    flags = row[0]
    if flags & ~3:
        return None
    fs, fn = int.from_bytes(row[1:9], "little", signed=True), int.from_bytes(row[9:13], "little", signed=True)
    us, un = int.from_bytes(row[13:21], "little", signed=True), int.from_bytes(row[21:25], "little", signed=True)
    f = (fs, fn) if flags & 1 else None
    u = (us, un) if flags & 2 else None
    return (f, u) if N.window_valid(f, u) else None


def extract_inputs(items, payload, tx_item_off, ref_cap, tx_status=None):
    """items: [(kind, data offset, len)]; returns (refs: list of 36-byte rows -- exactly what is
    written, at most ref_cap --, tx_ref_off [ntx + 1], tw_from [ntx], tw_until [ntx], gate [ntx])."""
    n_items, ntx = len(items), len(tx_item_off) - 1
    rows, tx_ref_off, tw_from, tw_until, gate = [], [], [], [], []
    start = 0  # the unclamped running count
    for t in range(ntx):
        i0, i1 = min(tx_item_off[t], n_items), min(tx_item_off[t + 1], n_items)
        mine, sides, flagged, windows = [], (None, None), False, 0
        for kind, off, length in items[i0:max(i0, i1)]:
            if kind == KIND_STATE_REF:
                b = _payload(payload, off, length, 36)
                if b is None:
                    flagged = True
                else:
                    mine.append(b)
            elif kind == KIND_TIME_WINDOW:
                b = _payload(payload, off, length, 25)
                w = _window(b) if b is not None else None
                windows += 1
                if w is None or windows > 1:
                    flagged = True
                else:
                    sides = w
        if flagged:
            mine, sides = [], (None, None)
        if start + len(mine) > ref_cap:
            flagged = True
        tx_ref_off.append(min(start, ref_cap))
        rows += mine[:max(0, min(start + len(mine), ref_cap) - min(start, ref_cap))]
        start += len(mine)
        tw_from.append(N.instant_ns(sides[0]))
        tw_until.append(N.instant_ns(sides[1]))
        st = tx_status[t] if tx_status is not None else 0
        gate.append(st if st else (TX_BAD_COMPONENT if flagged else 0))
    tx_ref_off.append(min(start, ref_cap))
    return rows, tx_ref_off, tw_from, tw_until, gate
