"""Writes ed25519_sign_vectors.json: Ed25519 signatures (RFC 8032, deterministic, as i2p's
EdDSAEngine makes them) from the Python oracle (oracle/i2p_ed25519.py sign), the expected
outputs of the keyed signer (cordahip_sign, K11).

Seeds: the keys the reference's tests derive with entropyToKeyPair(BigInteger.valueOf(e)),
e = 10, 20 .. 80 (TestConstants.kt: DUMMY_NOTARY_KEY 20, DUMMY_MAP_KEY 30, DUMMY_BANK_A_KEY
40, ...) through oracle.entropy_seed, and four seeded random seeds. Message lengths: the
block edges of the two SHA-512 inputs -- prefix || M (32 + len) and R || A || M (64 + len)
fill whole 128-byte blocks, padding included, at 47/48, 79/80, 175/176, 207/208 -- plus 1,
32 (a transaction id, the one-block fast paths) and 1000.

    python tests/golden/make_ed25519_sign_vectors.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import i2p_ed25519 as ed  # noqa: E402

LENGTHS = [1, 32, 47, 48, 79, 80, 175, 176, 207, 208, 1000]


def main():
    seeds = [("entropy_%d" % e, ed.entropy_seed(e)) for e in range(10, 81, 10)]
    seeds += [("random_%d" % i, hashlib.sha256(b"ed25519-sign-vectors seed %d" % i).digest()) for i in range(4)]
    keys, vectors = [], []
    for k, (name, seed) in enumerate(seeds):
        pub = ed.seed_to_keypair(seed)[0]
        keys.append({"name": name, "seed": seed.hex(), "pub": pub.hex()})
        for n in LENGTHS:
            msg = hashlib.shake_256(b"ed25519-sign-vectors msg %d %d" % (k, n)).digest(n)
            p, sig = ed.sign(seed, msg)
            assert p == pub and ed.verify_status(pub, sig, msg) == ed.OK
            vectors.append({"key": k, "msg": msg.hex(), "sig": sig.hex()})
    with open(os.path.join(HERE, "ed25519_sign_vectors.json"), "w") as f:
        json.dump({"source": "oracle/i2p_ed25519.py sign", "lengths": LENGTHS, "keys": keys, "vectors": vectors}, f,
                  indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
