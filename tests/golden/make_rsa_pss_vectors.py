"""Generates tests/golden/rsa_pss_vectors.json: RSA_SHA256 (RSASSA-PSS) keys and vectors,
each with the status bc_rsa_pss.py gives it under doVerify (`status`) and isValid
(`status_is_valid`) rules, pinned by the local OpenSSL (openssl_rsa_pss.py).

The assertion that pins them: on every vector whose key OpenSSL accepts, OpenSSL's verdict
equals the restatement's (taken without the GPU path's key declines and without the
emptiness checks, which OpenSSL does not have) -- EXCEPT the `top_bit` category, where the
restatement accepts and OpenSSL rejects (bc_rsa_pss.py). The count of exceptions must equal
the count of `top_bit` vectors; no other vector is skipped.

Keys are stored once and referred to by index; the test keys keep p, q and d so tests can
sign fresh messages by CRT. Run from the repository root: python tests/golden/make_rsa_pss_vectors.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bc_rsa_pss as bc  # noqa: E402
import openssl_rsa_pss as ossl  # noqa: E402

rng = random.Random(0x52534131)
SMALL = [p for p in range(3, 2000, 2) if all(p % q for q in range(3, int(p ** 0.5) + 1, 2))]


def is_prime(n):
    if n < 2 or n % 2 == 0:
        return n == 2
    for p in SMALL:
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d //= 2
        r += 1
    for _ in range(24):
        x = pow(rng.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def prime(bits, e):
    while True:
        p = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
        if gcd(p - 1, e) == 1 and is_prime(p):
            return p


def py_key(bits, e=65537, high=False):
    """A Miller-Rabin RSA key whose modulus has exactly `bits` bits (high: and its two top bits set)."""
    while True:
        p, q = prime((bits + 1) // 2, e), prime(bits // 2, e)
        n = p * q
        if p != q and n.bit_length() == bits and (not high or n >> (bits - 2) == 3):
            d = pow(e, -1, (p - 1) * (q - 1))
            return dict(n=n, e=e, d=d, p=p, q=q)


keys, vectors = [], []


def add_key(name, k=None, der=None):
    der = der if der is not None else bc.encode_key(k["n"], k["e"])
    rec = {"name": name, "der": der.hex()}
    for f in ("n", "e", "d", "p", "q"):
        if k and f in k:
            rec[f] = "%x" % k[f]
    keys.append(rec)
    return len(keys) - 1


def add(cat, ki, sig, msg):
    der = bytes.fromhex(keys[ki]["der"])
    vectors.append({"cat": cat, "key": ki, "sig": sig.hex(), "msg": msg.hex(),
                    "status": bc.verify(der, sig, msg), "status_is_valid": bc.verify(der, sig, msg, is_valid=True)})


def klen(k):
    return (k["n"].bit_length() + 7) // 8


def crt_sig(k, msg, **kw):
    """A CRT signature of msg with the given salt, or a fresh 32-byte one re-drawn until EM < n."""
    salt = kw.pop("salt", None)
    while True:
        em = bc.encode_em(msg, k["n"].bit_length(), rng.randbytes(32) if salt is None else salt, **kw)
        if em < k["n"]:
            return bc.sign_crt(em, k["p"], k["q"], k["d"]).to_bytes(klen(k), "big")
        assert salt is None


def msg(i):
    return ("rsa-pss golden message %d" % i).encode() * (1 + i % 4)


# ---- keys ------------------------------------------------------------------------
good = []  # (index, numbers, OpenSSL handle or None)
for bits in (2048, 3072, 4096, 2048):
    h, k = ossl.keygen(bits)
    good.append((add_key("openssl_%d%s" % (bits, "_b" if len(good) == 3 else ""), k), k, h))
for bits in (1024, 2049, 2056, 3071):
    k = py_key(bits, high=bits == 2049)  # room for m in [2^2048, n)
    good.append((add_key("py_%d" % bits, k), k, None))
for bits, e in ((2048, 3), (1536, 17), (3072, (1 << 32) - 1)):
    k = py_key(bits, e)
    good.append((add_key("py_%d_e%d" % (bits, e), k), k, None))
k0 = good[0][1]
declined = [
    (add_key("even_modulus", dict(n=k0["n"] + 1, e=k0["e"])), None),
    (add_key("py_1023", py_key(1023)), None),
    (add_key("py_4104", py_key(4104)), None),
    (add_key("even_e", dict(n=k0["n"], e=65536)), None),
    (add_key("py_1024_e2p32p1", py_key(1024, (1 << 32) + 1)), None),
]
der0 = bc.encode_key(k0["n"], k0["e"])
assert der0[1] == 0x82
body = k0["n"].to_bytes(256, "big")  # top bit set: reads as a negative INTEGER without its 00
neg = b"\x02\x82\x01\x00" + body + b"\x02\x03\x01\x00\x01"
three = der0[4:] + b"\x02\x01\x05"
malformed = [
    add_key("truncated", der=der0[:-1]),
    add_key("trailing_byte", der=der0 + b"\x00"),
    add_key("three_integers", der=b"\x30\x82" + len(three).to_bytes(2, "big") + three),
    add_key("negative_modulus", der=b"\x30\x82" + len(neg).to_bytes(2, "big") + neg),
    add_key("non_minimal_length", der=b"\x30\x83\x00" + der0[2:]),
]

# ---- vectors ---------------------------------------------------------------------
i = 0
for ki, k, h in good:
    for _ in range(2):
        m = msg(i)
        i += 1
        sig = ossl.sign(h, m) if h else crt_sig(k, m)  # OpenSSL's own signatures pin the happy path
        add("valid_openssl" if h else "valid", ki, sig, m)
    add("wrong_message", ki, sig, m + b"!")
    flipped = bytearray(sig)
    flipped[rng.randrange(len(sig))] ^= 1 << rng.randrange(8)
    add("bit_flip", ki, bytes(flipped), m)
    add("leading_zero_k_plus_1", ki, b"\x00" + sig, m)
    for s in (0, 1, k["n"] - 1, k["n"], k["n"] + 1):
        add("s_edge", ki, s.to_bytes(klen(k), "big"), m)
    add("trailer", ki, crt_sig(k, m, trailer=0xCC), m)
    add("salt_len_20", ki, crt_sig(k, m, salt=rng.randbytes(20)), m)
    add("nonzero_padding", ki, crt_sig(k, m, pad_byte=0x40), m)
    add("empty_signature", ki, b"", m)
    add("empty_message", ki, crt_sig(k, b""), b"")
# wrong key: a signature of one key under another of the same size
add("wrong_key", good[3][0], bytes.fromhex(vectors[0]["sig"]), bytes.fromhex(vectors[0]["msg"]))
add("wrong_key", good[0][0], crt_sig(good[3][1], msg(1)), msg(1))
# salt length 0: the separator is the last byte of DB
for ki, k, h in good[:1] + good[4:6]:
    add("salt_len_0", ki, crt_sig(k, msg(7), salt=b""), msg(7))
# a valid signature whose leading byte is zero, sent without it
for ki, k, h in (good[4], good[0]):
    while True:
        sig = crt_sig(k, msg(11))
        if sig[0] == 0:
            break
    add("stripped_leading_zero", ki, sig[1:], msg(11))
    add("valid", ki, sig, msg(11))
# m >= 2^(8 emLen): only where bits = 1 mod 8 (the 2049-bit key)
ki, k, h = good[5]
assert k["n"].bit_length() % 8 == 1
while True:  # a well-formed EM below the extra bit, so only rule 3 rejects it
    m_big = (1 << 2048) | bc.encode_em(msg(12), 2049, rng.randbytes(32))
    if m_big < k["n"]:
        break
assert bc.pss_check(m_big - (1 << 2048), 2049, msg(12)) and not bc.pss_check(m_big, 2049, msg(12))
add("m_above_em", ki, bc.sign_crt(m_big, k["p"], k["q"], k["d"]).to_bytes(klen(k), "big"), msg(12))
# BC-lenient: a bit of EM above emBits set (BC clears it after unmasking, RFC 8017 checks it)
n_top = 0
for ki, k, h in (good[0], good[1], good[4], good[6], good[7]):
    bits = k["n"].bit_length()
    assert (bits - 1) % 8, "the key has unused bits in EM[0]"
    add("top_bit", ki, crt_sig(k, msg(13), top_bits=1), msg(13))
    n_top += 1
# keys the GPU path declines (BC keeps them: UNSUPPORTED) and malformed keys (BAD_KEY)
for ki, _ in declined:
    rec = keys[ki]
    if "d" in rec:
        k = {f: int(rec[f], 16) for f in ("n", "e", "d", "p", "q")}
        add("declined_key_valid", ki, crt_sig(k, msg(14)), msg(14))
    add("declined_key", ki, bytes.fromhex(vectors[0]["sig"]), bytes.fromhex(vectors[0]["msg"]))
for ki in malformed:
    add("malformed_key", ki, bytes.fromhex(vectors[0]["sig"]), bytes.fromhex(vectors[0]["msg"]))
    add("malformed_key_empty", ki, b"", b"")

# ---- the pin: OpenSSL against the restatement ---------------------------------------
exceptions = rejected_keys = 0
for v in vectors:
    der, sig, m = bytes.fromhex(keys[v["key"]]["der"]), bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"])
    got = ossl.verify(der, sig, m)
    if got is None:  # OpenSSL does not take the key: the restatement must not either
        assert bc.decode_key(der, decline=False) == bc.BAD_KEY, v
        rejected_keys += 1
        continue
    want = bc.verify(der, sig, m, is_valid=True, decline=False) == bc.OK
    if v["cat"] == "top_bit":
        assert want and not got and v["status"] == bc.OK, v
        exceptions += 1
        continue
    assert got == want, (v["cat"], keys[v["key"]]["name"], got, want)
assert exceptions == n_top == sum(v["cat"] == "top_bit" for v in vectors)
assert rejected_keys == sum(keys[v["key"]]["name"] in ("truncated", "trailing_byte", "three_integers",
                                                       "negative_modulus", "non_minimal_length") for v in vectors)
cats = {}
for v in vectors:
    cats[v["cat"]] = cats.get(v["cat"], 0) + 1
out = os.path.join(HERE, "rsa_pss_vectors.json")
with open(out, "w") as f:
    json.dump({"comment": "RSA_SHA256 (RSASSA-PSS) vectors: tests/golden/make_rsa_pss_vectors.py; statuses by "
                          "bc_rsa_pss.py, pinned by OpenSSL except the top_bit category",
               "keys": keys, "vectors": vectors}, f, separators=(",", ":"))
print("%d keys, %d vectors, %d bytes; %d top_bit exceptions, %d vectors on keys OpenSSL rejects"
      % (len(keys), len(vectors), os.path.getsize(out), exceptions, rejected_keys))
print(cats)
