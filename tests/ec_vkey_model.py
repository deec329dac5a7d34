"""CPU model of the keyed ECDSA verifier (K13, corda_amd/csrc/ecdsa_vkey.hip), shared by
tests/test_ec_vkey_model.py and tests/test_gpu_ecdsa_verify_keyed.py. Not a test module.

Integer tables [d 256^j]X, d = 1..128, j = 0..31, built as the registration kernel builds
them (8 doublings per position, repeated addition within one) for the key AND for the base
point; the digit rule and the order of additions of ecdsa_vkey.hpp; the lane's sum
P = sum of table entries, then x(P) mod n == r. No scalar multiplication anywhere, so a
wrong base-point table, digit rule or sign would show. `trace` also reports which of the
mixed addition's exceptional branches a lane takes; `scalar_trace` finds them without any
point arithmetic for keys Q = [d]G with known d."""
import hashlib

import bc_ecdsa as bc

DIGITS, ENTRIES = 32, 128
BIAS = int.from_bytes(b"\x7f" * 32, "little")


def add(c, p1, p2):
    """Affine addition (None: infinity); bc_ecdsa._add with a faster inversion."""
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    (x1, y1), (x2, y2), p = p1, p2, c.p
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = (3 * x1 * x1 + c.a) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return (x3, (lam * (x1 - x3) - y1) % p)


def neg(c, pt):
    return None if pt is None else (pt[0], (c.p - pt[1]) % c.p)


def batch_add(c, pairs):
    """[p1 + p2 for (p1, p2) in pairs] for finite points with distinct x, with ONE inversion
    (Montgomery's trick over the denominators x2 - x1): the tables' 4,096 additions per key
    would otherwise cost 4,096 inversions."""
    p = c.p
    den = [(p2[0] - p1[0]) % p for p1, p2 in pairs]
    assert all(den)
    pre = [1]
    for x in den:
        pre.append(pre[-1] * x % p)
    inv = pow(pre[-1], -1, p)
    out = [None] * len(pairs)
    for i in range(len(pairs) - 1, -1, -1):
        di = inv * pre[i] % p  # 1 / den[i]
        inv = inv * den[i] % p
        (x1, y1), (x2, y2) = pairs[i]
        lam = (y2 - y1) * di % p
        x3 = (lam * lam - x1 - x2) % p
        out[i] = (x3, (lam * (x1 - x3) - y1) % p)
    return out


def point_table(c, base):
    """table[j][d] = [d 256^j]base, d = 1..128 (index 0 unused: a zero digit adds nothing):
    8 doublings per position, repeated addition of [256^j]base within one (all 32 positions
    advance together so that each step shares one inversion). d 256^j <= 2^255 < n, so no
    addition here meets equal x."""
    bases = []
    for _ in range(DIGITS):
        bases.append(base)
        for _ in range(8):
            base = add(c, base, base)
    table = [[None, b, add(c, b, b)] for b in bases]
    for _ in range(ENTRIES - 2):
        nxt = batch_add(c, [(row[-1], b) for row, b in zip(table, bases)])
        for row, e in zip(table, nxt):
            row.append(e)
    return table


_G_TABLES = {}


def g_table(scheme):
    if scheme not in _G_TABLES:
        c = bc.CURVES[scheme]
        _G_TABLES[scheme] = point_table(c, c.G)
    return _G_TABLES[scheme]


def digits(u: int, n: int):
    """ecdsa_vkey.hpp: (u', neg) = split_sign(u); byte j of u' + 0x7f7f..7f, minus 127."""
    assert 0 <= u < n
    negate = u >= 1 << 255
    up = n - u if negate else u
    assert up < 1 << 255
    t = up + BIAS
    assert t < 1 << 256  # no carry out
    d = [((t >> (8 * j)) & 0xff) - 127 for j in range(DIGITS)]
    assert sum(x << (8 * j) for j, x in enumerate(d)) == up and all(-127 <= x <= 128 for x in d)
    return d, negate


def additions(u1: int, u2: int, n: int):
    """The lane's additions in the header's order: (is_key, j, signed digit with the scalar's
    sign applied), j from 31 down to 0, the base point's entry then the key's; zero digits skipped."""
    d1, n1 = digits(u1, n)
    d2, n2 = digits(u2, n)
    out = []
    for j in range(DIGITS - 1, -1, -1):
        for is_key, d, ng in ((False, d1[j], n1), (True, d2[j], n2)):
            if d:
                out.append((is_key, j, -d if ng else d))
    return out, d1.count(0) + d2.count(0)


def trace(scheme, qtab, u1, u2):
    """The table sum and what it met: {'dbl': additions with the accumulator equal to the entry,
    'inf': additions that left the accumulator at infinity, 'zero': zero digits}."""
    c = bc.CURVES[scheme]
    gtab = g_table(scheme)
    adds, zeros = additions(u1, u2, c.n)
    ev = {"dbl": 0, "inf": 0, "zero": zeros}
    acc = None
    for is_key, j, d in adds:
        e = (qtab if is_key else gtab)[j][abs(d)]
        if d < 0:
            e = neg(c, e)
        if acc is not None and acc[0] == e[0]:
            ev["dbl" if acc[1] == e[1] else "inf"] += 1
        acc = add(c, acc, e)
    return acc, ev


def scalar_trace(n, dq, u1, u2):
    """`trace`'s events for the key Q = [dq]G, in the scalar domain (pure modular arithmetic)."""
    adds, zeros = additions(u1, u2, n)
    ev = {"dbl": 0, "inf": 0, "zero": zeros}
    acc = 0
    for is_key, j, d in adds:
        t = d * (1 << (8 * j)) * (dq if is_key else 1) % n
        if acc and acc == t:
            ev["dbl"] += 1
        elif acc and (acc + t) % n == 0:
            ev["inf"] += 1
        acc = (acc + t) % n
    return acc, ev


def scalars(scheme, sig: bytes, msg: bytes):
    """(r, u1, u2) of a signature that passed the DER and range checks."""
    n = bc.CURVES[scheme].n
    r, s = bc.der_decode(sig)
    e = int.from_bytes(hashlib.sha256(msg).digest(), "big") % n  # e < 2^256 < 2n: reduced once
    w = pow(s, -1, n)
    return r, e * w % n, r * w % n


def model_status(scheme, qtab, sig: bytes, msg: bytes, is_valid: bool = False):
    """The kernel's per-lane precedence for a registered key whose table is qtab; returns
    (status, events)."""
    n = bc.CURVES[scheme].n
    if not is_valid and (len(sig) == 0 or len(msg) == 0):
        return bc.EMPTY, None
    rs = bc.der_decode(sig)
    if rs is None:
        return bc.MALFORMED_SIG, None
    r, s = rs
    if not (1 <= r < n and 1 <= s < n):
        return bc.BAD_SIG, None
    r, u1, u2 = scalars(scheme, sig, msg)
    pt, ev = trace(scheme, qtab, u1, u2)
    if pt is None:
        return bc.BAD_SIG, ev
    return (bc.OK if pt[0] % n == r else bc.BAD_SIG), ev
