#!/usr/bin/env python3
"""Builds tests/golden/ecdsa_sign_vectors.json from tests/ecdsa_sign_model.py.

Keys on both curves (d = 1, d = n - 1, a d with leading zero bytes, two ordinary
ones), each signing one message of every SHA-256 padding edge (1, 31, 32, 55, 56, 63,
64, 119, 120, 200 bytes); then, per curve, 32-byte messages searched for what the
kernel's paths need: a nonce whose k' = min(k, n - k) has three zero top nibbles (the
accumulator stays at infinity past the first positions) and a signature of at most 69
bytes. properties() names what a case exercises; the CPU test asserts that every name
occurs for both curves.

    python3 tests/golden/make_ecdsa_sign_vectors.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ecdsa_sign_model as M  # noqa: E402

OUT = os.path.join(HERE, "ecdsa_sign_vectors.json")
LENGTHS = (1, 31, 32, 55, 56, 63, 64, 119, 120, 200)
REQUIRED = ("flip", "noflip", "top3zero", "midzero", "len72", "len71", "len70", "len<=69",
            "r_pad", "r_nopad", "s_pad", "s_nopad")


def message(tag, length):
    out, c = b"", 0
    while len(out) < length:
        out += hashlib.sha256(b"ecdsa-sign-vectors|%s|%d" % (tag.encode(), c)).digest()
        c += 1
    return out[:length]


def keys_of(c):
    mid = int.from_bytes(hashlib.sha256(b"ecdsa-sign-key|" + c.name.encode()).digest(), "big")
    return [1, c.n - 1, mid >> 40, mid % c.n, (mid * 3 + 7) % c.n]


def properties(c, k, r, s, sig):
    """What a case exercises, from its nonce and signature."""
    kp, flip = M.split_min(k, c.n)
    digits, _ = M.recode(kp)
    p = ["flip" if flip else "noflip"]
    if kp < 1 << 244:
        p.append("top3zero")
    if any(d == 0 for d in digits[16:48]):
        p.append("midzero")
    p.append("len%d" % len(sig) if len(sig) >= 70 else "len<=69")
    p.append("r_pad" if r.bit_length() % 8 == 0 else "r_nopad")
    p.append("s_pad" if s.bit_length() % 8 == 0 else "s_nopad")
    return p


def case(c, key_index, d, msg):
    r, s, k = M.sign_rs(c, d, msg)
    sig = M.der_sig(r, s)
    return {"key": key_index, "msg": msg.hex(), "sig": sig.hex(), "k": "%064x" % k,
            "props": properties(c, k, r, s, sig)}


def main():
    keys, cases = [], []
    for c in (M.K1, M.R1):
        base = len(keys)
        ds = keys_of(c)
        for d in ds:
            keys.append({"scheme": c.scheme, "d": "%064x" % d, "pub": M.public_key(c, d).hex()})
        for ki, d in enumerate(ds):
            for length in LENGTHS:
                cases.append(case(c, base + ki, d, message("%s|%d" % (c.name, ki), length)))
        # searched cases, with the curve's fourth key
        ki, d = 3, ds[3]
        want_top, want_short, i = True, True, 0
        while want_top or want_short:
            msg = message("%s|search|%d" % (c.name, i), 32)
            i += 1
            if want_top:  # the nonce alone decides: cheap
                k, _ = M.nonce(d, hashlib.sha256(msg).digest(), c.n)
                if M.split_min(k, c.n)[0] < 1 << 244:
                    cases.append(case(c, base + ki, d, msg))
                    want_top = False
                    continue
            if want_short:
                cs = case(c, base + ki, d, msg)
                if "len<=69" in cs["props"]:
                    cases.append(cs)
                    want_short = False
    assert len(cases) <= 400
    for c in (M.K1, M.R1):
        have = set()
        for cs in cases:
            if keys[cs["key"]]["scheme"] == c.scheme:
                have.update(cs["props"])
        missing = [p for p in REQUIRED if p not in have]
        assert not missing, (c.name, missing)
    with open(OUT, "w") as f:
        json.dump({"lengths": list(LENGTHS), "keys": keys, "cases": cases}, f, indent=0)
        f.write("\n")
    print("%d keys, %d cases -> %s" % (len(keys), len(cases), OUT))


if __name__ == "__main__":
    main()
