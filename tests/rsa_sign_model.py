"""What the RSA signing tests share: the golden keys that keep their private parts
(tests/golden/rsa_pss_vectors.json), their CRT components, the Python restatement of a lane
(bc_rsa_pss.encode_em followed by sign_crt, as k bytes) and the keys an add must turn down."""
import json
import os
import random

import bc_rsa_pss as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# declined by the verifier's own rules, so by the signer too
DECLINED = ("py_1023", "py_4104", "py_1024_e2p32p1")
MSG_LENS = (1, 32, 55, 56, 64, 200)


def class_words(bits):
    return 64 if bits <= 2048 else 96 if bits <= 3072 else 128


class Key:
    def __init__(self, name, p, q, d, e):
        self.name, self.p, self.q, self.d, self.e = name, p, q, d, e
        self.n = p * q
        self.bits = self.n.bit_length()
        self.k = (self.bits + 7) // 8
        self.dp, self.dq, self.qinv = d % (p - 1), d % (q - 1), pow(q, -1, p)

    @property
    def words(self):
        return class_words(self.bits)

    def crt(self):
        return self.p, self.q, self.dp, self.dq, self.qinv

    def sign(self, msg: bytes, salt: bytes) -> bytes:
        return bc.sign_crt(bc.encode_em(msg, self.bits, salt), self.p, self.q, self.d).to_bytes(self.k, "big")

    def der(self):
        return bc.encode_key(self.n, self.e)


def private_keys():
    """every golden key with p, q and d, in file order"""
    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        keys = json.load(f)["keys"]
    return [Key(k["name"], int(k["p"], 16), int(k["q"], 16), int(k["d"], 16), int(k["e"], 16))
            for k in keys if "p" in k]


def accepted_keys():
    return [k for k in private_keys() if k.name not in DECLINED]


def message(i: int, n: int) -> bytes:
    return random.Random(0x19000 + 131 * i + n).randbytes(n)


def salt(i: int) -> bytes:
    return random.Random(0x5a17 + i).randbytes(32)


def rejected_keys(k: Key):
    """(what, (p, q, dp, dq, qinv) with None for a zero-length component, e, the add's status) for
    every key an add must turn down, made from the accepted key k. BAD_KEY "by consistency": the
    record builds and the consistency run fails."""
    p, q, dp, dq, qinv = k.crt()
    rng = random.Random(0x19)
    w = k.words
    big = rng.getrandbits(16 * w + 16) | 1 | (1 << (16 * w + 15))    # unbalanced: the larger prime 16 bits above
    small = rng.getrandbits(16 * w - 24) | 1 | (1 << (16 * w - 25))  # 16 W, the modulus still in the class
    assert class_words((big * small).bit_length()) == k.words and big.bit_length() > 16 * k.words
    out = [("zero-length p", (None, q, dp, dq, qinv), k.e, bc.BAD_KEY),
           ("zero-length dq", (p, q, dp, None, qinv), k.e, bc.BAD_KEY),
           ("zero-length qinv", (p, q, dp, dq, None), k.e, bc.BAD_KEY),
           ("p even", (p + 1, q, dp, dq, qinv), k.e, bc.BAD_KEY),
           ("q even", (p, q - 1, dp, dq, qinv), k.e, bc.BAD_KEY),
           ("p = 1", (1, q, 0, dq, 0), k.e, bc.BAD_KEY),
           ("q = 0", (p, 0, dp, 0, qinv), k.e, bc.BAD_KEY),
           ("p = q", (p, p, dp, dp, qinv), k.e, bc.BAD_KEY),
           ("e even", (p, q, dp, dq, qinv), k.e + 1, bc.BAD_KEY),
           ("e = 1", (p, q, dp, dq, qinv), 1, bc.BAD_KEY),
           ("dP >= p", (p, q, dp + p, dq, qinv), k.e, bc.BAD_KEY),
           ("dP = p", (p, q, p, dq, qinv), k.e, bc.BAD_KEY),
           ("dQ >= q", (p, q, dp, dq + q, qinv), k.e, bc.BAD_KEY),
           ("qInv >= p", (p, q, dp, dq, qinv + p), k.e, bc.BAD_KEY),
           ("dQ + 2", (p, q, dp, dq + 2, qinv), k.e, "consistency"),
           ("qInv + 1", (p, q, dp, dq, qinv + 1), k.e, "consistency"),
           ("dP + 2", (p, q, dp + 2, dq, qinv), k.e, "consistency"),
           ("unbalanced", (big, small, 1, 1, 1), k.e, bc.UNSUPPORTED)]
    assert dq + 2 < q and qinv + 1 < p and dp + 2 < p
    return out
