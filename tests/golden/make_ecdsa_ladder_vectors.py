#!/usr/bin/env python3
"""Generate tests/golden/ecdsa_ladder_vectors.json (secp256k1 = scheme 2, P-256 = 3): signatures
built so that the generic ECDSA verifier's ladder (K2, ecdsa_ladder_lane in corda_amd/csrc/ecdsa.hip)
meets the exceptional branches of its point additions and the ends of its digit ranges, which a
random signature reaches with probability about 2^-256. tests/ec_ladder_model.py states the ladder's
schedule; every vector records the events that model sees and the key's scalar d (Q = [d]G), from
which tests/test_ec_ladder_model.py derives the events again.

Every valid lane satisfies u1 + d u2 = k with r = x([k]G) mod n, for a key Q = [d]G:

  dbl G / dbl LG   the ladder's last addition is a G-table (lambda-G-table) entry [g]G that equals the
                   accumulator: k = 2g (2 g lambda), u1 chosen with g as its last digit, then
                   u2 = u1 r / e, d = (k - u1) / u2, s = r / u2. No search.
  inf              keys d = 1 and d = n - 1 with a short nonce: the top digits of u1 and of +-u2 cancel,
                   the sum passes through infinity (accumulator = -addend), a window's doublings run on
                   infinity and the next addition restarts from it. Messages are searched in the scalar
                   domain; the nonce length moves the window at which the sum vanishes.
  final_inf        arbitrary r, s and Q = [-e / r]G: the sum ends at infinity, status BAD_SIG.
  u1 = x, u2 = x   chosen scalars (known k, then d = (k - u1) / u2): the keyed test's fixed scalars,
                   nibble and bit patterns, secp256k1's lambda and lattice basis values, the scalars
                   with the longest GLV halves (128 bits, see split_extremes), and digit patterns that put
                   |digit| = 8 on every per-lane table and |digit| = 2^19 on every G table.

No lane with a `dbl` at a per-lane Q-table addition is included: e is a hash value, so a Q-table
entry that equals the accumulator fixes u2 up to about 24 bits of conditions once k and the message
are chosen, and every route found costs about 2^16 point multiplications or 2^24 hashes per vector.

For every vector the script asserts that oracle/bc_ecdsa.verify_status gives the stated status, that
OpenSSL 3 ECDSA_verify agrees (1 for OK; it rejects a sum at infinity with its error value -1), and
that the model's point trace and scalar trace report the same events (and, for a valid lane, a point whose x mod n is r). The output is deterministic.
"""
import hashlib
import json
import os
import sys
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import bc_ecdsa as ec  # noqa: E402
import ec_ladder_model as model  # noqa: E402
import openssl_ecdsa as ossl  # noqa: E402

K1, R1 = model.K1, model.R1
# ECDSA_verify: 1 for a valid lane. For a sum at infinity OpenSSL fails to read the point's affine
# coordinates and returns its error value -1, where BouncyCastle's ECDSASigner returns false (BAD_SIG):
# both reject, and the -1 is asserted as such.
OSSL = {ec.OK: 1, ec.BAD_SIG: -1}
FIXED_SCALARS = ["1", "n-1", "2^255-1", "2^255", "2^255+1", "0x80..", "0x81..", "0xff.."]
# nonce lengths (bits) for the `inf` lanes: each shorter one makes the sum vanish at one more G window
INF_NONCE_BITS = {R1: (231, 211, 131), K1: (115, 95, 55)}
INF_PER_CELL = 2  # lanes per (nonce length, key)
vectors = []


def h256(tag: bytes) -> int:
    return int.from_bytes(hashlib.sha256(tag).digest(), "big")


def message(tag: bytes) -> bytes:
    return hashlib.sha256(b"ec-ladder-msg-" + tag).digest()


def e_of(msg: bytes, n: int) -> int:
    return int.from_bytes(hashlib.sha256(msg).digest(), "big") % n


def pub_of(scheme, d):
    x, y = model.mul(ec.CURVES[scheme], d, ec.CURVES[scheme].G)
    return b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big")


def r_of(scheme, k):
    c = ec.CURVES[scheme]
    return model.mul(c, k, c.G)[0] % c.n


def add(scheme, d, r, s, msg, status, what, need=()):
    """Record one lane on the key [d]G; `need`: events the lane must show."""
    c = ec.CURVES[scheme]
    pub, sig = pub_of(scheme, d), ec.der_encode(r, s)
    assert ec.verify_status(scheme, pub, sig, msg) == status, (what, status)
    o = ossl.verify(scheme, pub, sig, msg)
    assert o == OSSL[status], (what, status, o)
    rr, u1, u2 = model.scalars(scheme, sig, msg)
    acc, sev = model.scalar_trace(scheme, d, u1, u2)
    pt, pev = model.trace(scheme, ec.decode_point(c, pub), u1, u2)
    assert pev == sev, (what, pev, sev)
    assert acc == (u1 + d * u2) % c.n
    if status == ec.OK:
        assert pt is not None and pt[0] % c.n == rr == r, what
    else:
        assert pt is None and acc == 0, what
    for name in need:
        assert model.has(sev, *name), (what, name, sev)
    vectors.append({"scheme": scheme, "pub": pub.hex(), "sig": sig.hex(), "msg": msg.hex(), "status": status,
                    "openssl": o, "d": "%064x" % d, "events": [list(x) for x in sev], "for": what})
    return sev


def chosen(scheme, k, r, msg, what, u1=None, u2=None, need=()):
    """The lane with the given u1 (or u2) and nonce k: s from the scalar, then d = (k - u1) / u2."""
    n = ec.CURVES[scheme].n
    e = e_of(msg, n)
    assert e
    if u1 is not None:
        s = e * pow(u1, -1, n) % n
        u2 = r * pow(s, -1, n) % n
    else:
        s = r * pow(u2, -1, n) % n
        u1 = e * pow(s, -1, n) % n
    d = (k - u1) * pow(u2, -1, n) % n
    assert d and s
    return add(scheme, d, r, s, msg, ec.OK, what, need)


def fixed_scalars(n):
    return [1, n - 1, (1 << 255) - 1, 1 << 255, (1 << 255) + 1, int.from_bytes(b"\x80" * 32, "big") % n,
            int.from_bytes(b"\x81" * 32, "big") % n, int.from_bytes(b"\xff" * 32, "big") % n]


def q_pattern(nbytes):
    """Nibbles 0, 7, then 8, 7 alternating down to the lowest: a 7 above an 8 recodes to +8, an 8 above a
    7 to -8 (booth_digit<4>)."""
    return int.from_bytes(b"\x07" + b"\x87" * (nbytes - 1), "big")


def g_pattern(chunks):
    """20-bit chunks 0x80000 (even positions) and 0x7ffff (odd): -2^19 and +2^19 (booth_digit<20>)."""
    return sum((0x80000 if i % 2 == 0 else 0x7ffff) << (20 * i) for i in range(chunks))


def glv_join(a1, a2, n):
    u = (a1 + a2 * model.LAMBDA) % n
    assert model.glv_split(u) == (a1, a2), (hex(a1), hex(a2))
    return u


def split_extremes(n):
    """The scalars with the longest GLV halves, one with such a half non-negative and one with it
    negative. The halves of k are k minus the nearest lattice point, so they are longest next to the
    corners (+-v1 +- v2) / 2 of the basis cell, v1 = (A1, B1), v2 = (A2, B2): those are searched through
    the model. With this basis the longest half has 128 bits (|r1| <= (|A1| + |A2|) / 2 < 2^128 and
    |r2| <= (|B1| + |B2|) / 2 < 2^128), one bit below the 129 the kernel's 33 windows allow for."""
    g = model.gen
    best = {}
    for s1 in (1, -1):
        for s2 in (1, -1):
            for t1 in range(-2, 3):
                for t2 in range(-2, 3):
                    u = ((s1 * g.A1 + s2 * g.A2) // 2 + t1 + ((s1 * g.B1 + s2 * g.B2) // 2 + t2) * model.LAMBDA) % n
                    for r in model.glv_split(u):
                        mag, negative = model.split_sign(r, n)
                        key = "split-max-" if negative else "split-max+"
                        if key not in best or mag > best[key][0]:
                            best[key] = (mag, u)
    assert all(best[k][0].bit_length() == 128 for k in best), best
    return [("split-max+", best["split-max+"][1]), ("split-max-", best["split-max-"][1])]


for scheme in (K1, R1):
    c = ec.CURVES[scheme]
    n = c.n

    # ---- dbl at a G-table addition ------------------------------------------------------------
    for table in ("G", "LG") if scheme == K1 else ("G",):
        for i in range(10):
            tag = b"dbl-%d-%s-%d" % (scheme, table.encode(), i)
            g = 1 + h256(b"ec-ladder-g-" + tag) % ((1 << 19) - 1)
            rnd = h256(b"ec-ladder-u1-" + tag)
            if scheme == R1:
                k = 2 * g
                u1 = ((rnd >> 21) << 20) | g  # below 2^255, last 20-bit digit g
            else:
                hi = ((rnd >> 136) >> 20) << 20, (((rnd >> 16) & ((1 << 120) - 1)) >> 20) << 20
                if table == "G":
                    k = 2 * g
                    u1 = glv_join(hi[0] | g, hi[1], n)  # the lambda-G half's last digit is zero
                else:
                    k = 2 * g * model.LAMBDA % n
                    u1 = glv_join(hi[0] | (rnd & 0xfffff), hi[1] | g, n)
            ev = chosen(scheme, k, r_of(scheme, k), message(tag), "dbl " + table, u1=u1, need=[("dbl", table)])
            assert ev[-1] == ("dbl", 0, table)  # the ladder's last addition

    # ---- through infinity in the middle of the ladder ----------------------------------------
    windows = set()
    for bits in INF_NONCE_BITS[scheme]:
        k = h256(b"ec-ladder-nonce-%d-%d" % (scheme, bits)) >> (256 - bits) | 1 << (bits - 1)
        r, kinv = r_of(scheme, k), pow(k, -1, n)
        for d in (1, n - 1):
            got = i = 0
            while got < INF_PER_CELL:
                assert i < 2000, (scheme, bits, d)
                msg = message(b"inf-%d-%d-%d-%d" % (scheme, bits, d & 1, i))
                i += 1
                s = kinv * (e_of(msg, n) + r * d) % n
                if not s:
                    continue
                w = pow(s, -1, n)
                _, ev = model.scalar_trace(scheme, d, e_of(msg, n) * w % n, r * w % n)  # the search: scalars alone
                if not all(model.has(ev, x) for x in ("inf", "dbl_of_inf", "from_inf")):
                    continue
                add(scheme, d, r, s, msg, ec.OK, "inf nonce<2^%d d=%s" % (bits, "1" if d == 1 else "n-1"),
                    need=[("inf",), ("dbl_of_inf",), ("from_inf",)])
                windows.update(x[1] for x in model.has(ev, "inf"))
                got += 1
    assert len(windows) >= 2, windows

    # ---- a sum that ends at infinity ----------------------------------------------------------
    for i in range(4):
        msg = message(b"final-inf-%d-%d" % (scheme, i))
        r = 1 + h256(b"ec-ladder-final-r-%d-%d" % (scheme, i)) % (n - 1)
        s = 1 + h256(b"ec-ladder-final-s-%d-%d" % (scheme, i)) % (n - 1)
        ev = add(scheme, -e_of(msg, n) * pow(r, -1, n) % n, r, s, msg, ec.BAD_SIG, "final_inf", need=[("final_inf",)])
        assert ev[-2][0] == "inf" and ev[-1][0] == "final_inf"  # reached through the last addition

    # ---- chosen scalars -------------------------------------------------------------------------
    named = list(zip(FIXED_SCALARS, fixed_scalars(n)))
    named += [("0x88..", int.from_bytes(b"\x88" * 32, "big") % n), ("0x77..", int.from_bytes(b"\x77" * 32, "big")),
              ("2^240", 1 << 240), ("2^20-1", (1 << 20) - 1)]
    if scheme == K1:
        named += [("lambda", model.LAMBDA), ("n-lambda", n - model.LAMBDA), ("A1", model.gen.A1), ("A2", model.gen.A2),
                  ("n-A1", n - model.gen.A1), ("2^128", 1 << 128), ("2^128-1", (1 << 128) - 1)]
        named += split_extremes(n)
        named += [("qmax", glv_join(q_pattern(15), q_pattern(15), n)), ("gmax", glv_join(g_pattern(6), g_pattern(6), n))]
    else:
        named += [("qmax", q_pattern(32)), ("gmax", g_pattern(12))]
    k = h256(b"ec-ladder-chosen-nonce-%d" % scheme) % n
    r = r_of(scheme, k)
    for name, u in named:
        assert 0 < u < n
        for which in (1, 2):
            msg = message(b"chosen-%d-%s-%d" % (scheme, name.encode(), which))
            need = []
            if name == "qmax" and which == 2:
                need = [("qmax", t) for t in model.TABLES[scheme] if t in ("Q", "PQ")]
            if name == "gmax" and which == 1:
                need = [("gmax", t) for t in model.TABLES[scheme] if t in ("G", "LG")]
            chosen(scheme, k, r, msg, "u%d = %s" % (which, name), need=need, **{"u%d" % which: u})

with open(os.path.join(HERE, "ecdsa_ladder_vectors.json"), "w") as f:
    f.write('{"generator": "tests/golden/make_ecdsa_ladder_vectors.py",\n'
            '"oracle": "oracle/bc_ecdsa.py (BouncyCastle 1.57 SHA256withECDSA restatement)",\n'
            '"independent": "OpenSSL 3 ECDSA_verify",\n"model": "tests/ec_ladder_model.py",\n"vectors": [\n')
    f.write(",\n".join(json.dumps(v, separators=(",", ":")) for v in vectors))
    f.write("\n]}\n")
count = Counter()
for v in vectors:
    for key in {(v["scheme"], x[0], x[2]) for x in v["events"]}:
        count[key] += 1
print(len(vectors), "vectors; lanes per (scheme, event, table):")
for key in sorted(count, key=str):
    print("  ", key, count[key])
