#!/usr/bin/env python3
"""Generate tests/golden/pmt_build_vectors.json: FilteredTransaction build cases
(cordahip_filtered_tx_build).

Each case: a transaction's leaf preimages, one include flag per leaf (the filter
predicate's verdict), and what FilteredTransaction.buildMerkleTransaction
(MerkleTransaction.kt:121-128) makes of them: the status (0 built, 6
MerkleTreeException for no leaves, 12 MerkleTreeException "Some of the provided
hashes are not in the tree", PartialMerkleTree.kt:75-76), the root and the
PartialMerkleTree as its post-order token stream.

Expected values come from oracle/partial_merkle.py alone (merkle_tree, build,
tokens, restating MerkleTree.kt:27-66 and PartialMerkleTree.kt:68-125); the mask
becomes includeHashes as filterWithFun does it: the hashes of the flagged
leaves, in order, duplicates kept. The first block restates the reference's own
PartialMerkleTreeTest.kt cases on leaves 'a'..'f' serialised as in
make_pmt_vectors.py.
"""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import partial_merkle as pm  # noqa: E402

H = lambda b: hashlib.sha256(b).digest()  # noqa: E731
kryo_char = lambda c: b"corda\x00\x00\x01" + bytes([7]) + ord(c).to_bytes(2, "big")  # noqa: E731


def case(name, leaves, mask, note=""):
    assert len(leaves) == len(mask)
    hs = [H(x) for x in leaves]
    if not leaves:
        status, root, toks = 6, bytes(32), []  # MerkleTree.kt:49-50; the id as cordahip_tx_ids writes it
    else:
        tree = pm.merkle_tree(hs)
        root = tree[1]
        try:
            toks = pm.tokens(pm.build(tree, [h for h, f in zip(hs, mask) if f]))
            status = 0
        except pm.MerkleTreeException:
            toks, status = [], 12
    return {"name": name, "leaves": [x.hex() for x in leaves], "include": [1 if f else 0 for f in mask],
            "status": status, "root": root.hex(), "tokens": [[t, h.hex() if h else None] for t, h in toks],
            "note": note}


def generate():
    cases = []
    pre = [kryo_char(c) for c in "abcdef"]
    # PartialMerkleTreeTest.kt:143-147 (leaves 3 and 5), :156-159 (all), :150-153 / `nothing filtered` (none)
    cases.append(case("ref_3_5", pre, [i in (3, 5) for i in range(6)]))
    cases.append(case("ref_all", pre, [True] * 6))
    cases.append(case("ref_none", pre, [False] * 6, "the single token Leaf(rootHash); verify() is what throws"))
    # :167-173 only duplicate leaves, less included failure; and all three flagged
    aaa = [kryo_char("a")] * 3
    cases.append(case("aaa_first", aaa, [True, False, False], "PartialMerkleTreeTest.kt:167-173"))
    cases.append(case("aaa_all", aaa, [True, True, True]))
    # equal leaves in different subtrees of an 8-leaf tree
    eight = [kryo_char(c) for c in "abcdebgh"]
    cases.append(case("eight_dup_one", eight, [i == 1 for i in range(8)], "leaf 5 equals the flagged leaf 1"))
    cases.append(case("eight_dup_both", eight, [i in (1, 5) for i in range(8)]))
    # one leaf (MerkleTree.kt:51-52: the tree is that leaf), no leaves
    cases.append(case("one_flagged", [pre[0]], [True]))
    cases.append(case("one_unflagged", [pre[0]], [False]))
    cases.append(case("no_leaves", [], []))

    rng = random.Random(0xF17E4ED)

    def leaves_of(n):  # lengths as in make_pmt_vectors.py; the index prefix keeps the leaves distinct
        return [(bytes([j]) if n <= 256 else j.to_bytes(2, "little"))
                + bytes(rng.getrandbits(8) for _ in range(rng.choice([0, 42, 54, 63, 139]))) for j in range(n)]

    for m in range(1, 35):
        dens = rng.choice([0.1, 0.3, 0.5, 0.9])
        cases.append(case("random_m%d" % m, leaves_of(m), [rng.random() < dens for _ in range(m)]))
    # the slot bound reached and nearly doubled: 2 * 32 - 1 and 2 * 64 - 1 tokens
    cases.append(case("full_32", leaves_of(32), [True] * 32))
    cases.append(case("full_33", leaves_of(33), [True] * 33))
    cases.append(case("thousand_ends", leaves_of(1000), [i in (0, 999) for i in range(1000)]))
    return {"generator": "tests/golden/make_pmt_build_vectors.py", "cases": cases}


def dumps(doc):
    return json.dumps(doc, indent=0)


if __name__ == "__main__":
    doc = generate()
    with open(os.path.join(HERE, "pmt_build_vectors.json"), "w") as f:
        f.write(dumps(doc))
    print(len(doc["cases"]), "cases")
