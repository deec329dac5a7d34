"""tests/golden/ed25519_sign_vectors.json (made by the Python oracle) against the two
other independent signers in the tree: the C oracle (oracle_ed25519_sign /
oracle_ed25519_keypair) and, where libcrypto loads, OpenSSL. Ed25519 signing is
deterministic, so all three must agree byte for byte; the GPU signer is then held to
the same file (tests/test_gpu_sign.py)."""
import ctypes
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [1, 32, 47, 48, 79, 80, 175, 176, 207, 208, 1000]


def load_sign_vectors():
    with open(os.path.join(HERE, "golden", "ed25519_sign_vectors.json")) as f:
        j = json.load(f)
    keys = [dict(k, seed=bytes.fromhex(k["seed"]), pub=bytes.fromhex(k["pub"])) for k in j["keys"]]
    vecs = [dict(key=v["key"], msg=bytes.fromhex(v["msg"]), sig=bytes.fromhex(v["sig"])) for v in j["vectors"]]
    return keys, vecs


@pytest.fixture(scope="module")
def vectors():
    return load_sign_vectors()


def test_file_covers_the_block_edges(vectors):
    import i2p_ed25519 as ed
    keys, vecs = vectors
    assert [k["name"] for k in keys][:8] == ["entropy_%d" % e for e in range(10, 81, 10)]
    assert [k["seed"] for k in keys][:8] == [ed.entropy_seed(e) for e in range(10, 81, 10)]
    assert len(keys) >= 12 and len({k["seed"] for k in keys}) == len(keys)
    for k in range(len(keys)):
        assert [len(v["msg"]) for v in vecs if v["key"] == k] == LENGTHS
    assert os.path.getsize(os.path.join(HERE, "golden", "ed25519_sign_vectors.json")) < 256 * 1024


def test_python_oracle_reproduces_the_file(vectors):
    import i2p_ed25519 as ed
    keys, vecs = vectors
    for k in keys:
        assert ed.seed_to_keypair(k["seed"])[0] == k["pub"]
    for v in vecs[::7]:
        assert ed.sign(keys[v["key"]]["seed"], v["msg"]) == (keys[v["key"]]["pub"], v["sig"])


def test_c_oracle_agrees(vectors, oracle):
    keys, vecs = vectors
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    for k in keys:
        oracle.oracle_ed25519_keypair(k["seed"], pub)
        assert pub.raw == k["pub"], k["name"]
    for v in vecs:
        k = keys[v["key"]]
        oracle.oracle_ed25519_sign(k["seed"], v["msg"], len(v["msg"]), pub, sig)
        assert pub.raw == k["pub"] and sig.raw == v["sig"], (k["name"], len(v["msg"]))
        assert oracle.oracle_ed25519_verify(k["pub"], 32, v["sig"], 64, v["msg"], len(v["msg"])) == 0


def test_openssl_agrees(vectors):
    import openssl_ed25519 as ossl
    if not ossl.available():
        pytest.skip("libcrypto does not load")
    keys, vecs = vectors
    for k in keys:
        assert ossl.keypair(k["seed"]) == k["pub"], k["name"]
    for v in vecs:
        k = keys[v["key"]]
        assert ossl.sign(k["seed"], v["msg"]) == v["sig"], (k["name"], len(v["msg"]))
