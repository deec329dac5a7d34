"""corda_amd.corpus.cash_payment_items on the CPU: deterministic from its seed, every
transaction in availableComponents order, inputs that spend issue ids first and then
outputs of earlier transactions, never twice; its ids are the Merkle roots over the MODEL's
leaves (tests/kryo_payment_model.py) of its own components."""
import hashlib

import numpy as np

import kryo_payment_model as M
from corda_amd import _lib
from corda_amd.corpus import cash_payment_items, merkle_root

KEYS = np.frombuffer(b"".join(hashlib.sha256(b"k%d" % i).digest() for i in range(12)), np.uint8).reshape(12, 32)
NOTARY = bytes(range(32))


def test_payment_corpus_shape_and_ids():
    c = cash_payment_items(KEYS, NOTARY, 200, 11, window_frac=0.4, with_components=True)
    d = cash_payment_items(KEYS, NOTARY, 200, 11, window_frac=0.4)
    assert np.array_equal(c["blob"], d["blob"]) and np.array_equal(c["items"], d["items"])
    assert np.array_equal(c["ids"], d["ids"]) and not d["components"]
    assert not np.array_equal(c["ids"], cash_payment_items(KEYS, NOTARY, 200, 12)["ids"])
    order = ["state_ref", "cash_state", "move_command", "party", "ed25519_key", "kotlin_object", "time_window"]
    ids, spent, earlier = [bytes(x) for x in c["ids"]], set(), 0
    for t, comps in enumerate(c["components"]):
        kinds = [k for k, _, _ in comps]
        assert kinds == sorted(kinds, key=order.index)
        n = {k: kinds.count(k) for k in order}
        assert 1 <= n["state_ref"] <= 3 and 1 <= n["cash_state"] <= 2 and n["move_command"] == n["party"] == 1
        assert n["kotlin_object"] == 1 and n["time_window"] == (c["windows"][t] is not None)
        sg = c["signers"][t]
        assert n["ed25519_key"] == len(sg) + 1 and len(set(sg)) == len(sg)
        _, keys, h, al = M.unpack_move_command(comps[kinds.index("move_command")][1])
        assert [k for _, k in keys] == [KEYS[o].tobytes() for o in sg] and h is None and al
        leaves = [M.component_leaf(*comp) for comp in comps]
        assert merkle_root([hashlib.sha256(x).digest() for x in leaves]) == ids[t]
        a, b = int(c["tx_item_off"][t]), int(c["tx_item_off"][t + 1])
        assert [int(k) for k in c["items"]["kind"][a:b]] == [_lib.KRYO_KINDS[k] for k in kinds]
        for ref in c["refs"][t]:
            assert ref not in spent  # no double spend inside the corpus
            spent.add(ref)
            earlier += ref[0] in ids[:t]
            assert ref[0] not in ids[t:]
    assert earlier > 20 and sum(w is not None for w in c["windows"]) > 40
    assert 0 < sum(w is not None and w[0] is None for w in c["windows"])  # one-sided windows too
