"""Pure-Python model of ECDSA signing with registered keys (kernel K17).

Per lane (include/cordahip.h, cordahip_ecdsa_sign): h1 = SHA-256(m); k is the
RFC 6979 3.2 nonce (HMAC-SHA256, x = int2octets(d), bits2octets(h1) = int(h1) mod n);
candidates with k = 0, k >= n, r = 0 or s = 0 are passed over by the h.3 update;
r = x([k]G) mod n, s = k^-1 (e + d r) mod n with e = int(h1) mod n, s not normalised;
the output is the minimal DER SEQUENCE { INTEGER r, INTEGER s }. The modulus is a
parameter of the nonce function, so the retry path can be exercised with a modulus
that rejects half of all candidates.

Also here: the split k' = min(k, n - k), the signed 4-bit recoding, and the
branch-free mixed addition's selection rule over affine points, as the kernel
applies them (top digit first), with a check that the general addition never meets
a doubling or an inverse.
"""
import hashlib
import hmac

MAX_TRIES = 8


class Curve:
    def __init__(self, scheme, name, p, a, b, gx, gy, n):
        self.scheme, self.name, self.p, self.a, self.b, self.gx, self.gy, self.n = scheme, name, p, a, b, gx, gy, n

    @property
    def G(self):
        return (self.gx, self.gy)


K1 = Curve(
    2, "secp256k1", 2**256 - 2**32 - 977, 0, 7,
    0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
    0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8,
    0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141)
R1 = Curve(
    3, "secp256r1", 2**256 - 2**224 + 2**192 + 2**96 - 1, -3,
    0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B,
    0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
    0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5,
    0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551)
CURVES = {2: K1, 3: R1}


# ---- affine group law (None: the point at infinity) ---------------------------
def add(c, P, Q):
    if P is None:
        return Q
    if Q is None:
        return P
    p = c.p
    if P[0] == Q[0]:
        if (P[1] + Q[1]) % p == 0:
            return None
        lam = (3 * P[0] * P[0] + c.a) * pow(2 * P[1], -1, p) % p
    else:
        lam = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
    x = (lam * lam - P[0] - Q[0]) % p
    return (x, (lam * (P[0] - x) - P[1]) % p)


def neg(c, P):
    return None if P is None else (P[0], (-P[1]) % c.p)


def mul(c, k, P):
    R = None
    while k:
        if k & 1:
            R = add(c, R, P)
        P = add(c, P, P)
        k >>= 1
    return R


def public_key(c, d):
    """SEC1 uncompressed [d]G."""
    x, y = mul(c, d, c.G)
    return b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big")


# ---- RFC 6979 -------------------------------------------------------------------
def _hm(K, data):
    return hmac.new(K, data, hashlib.sha256).digest()


def nonce_candidates(d, h1, q):
    """The stream of candidates for key d and digest h1 under modulus q."""
    x = d.to_bytes(32, "big")
    h = (int.from_bytes(h1, "big") % q).to_bytes(32, "big")
    K, V = b"\x00" * 32, b"\x01" * 32
    K = _hm(K, V + b"\x00" + x + h)
    V = _hm(K, V)
    K = _hm(K, V + b"\x01" + x + h)
    V = _hm(K, V)
    while True:
        V = _hm(K, V)
        yield int.from_bytes(V, "big")
        K = _hm(K, V + b"\x00")
        V = _hm(K, V)


def nonce(d, h1, q, max_tries=MAX_TRIES):
    """(k, tries): the first candidate in [1, q - 1] among max_tries; (None, max_tries) when none is."""
    gen = nonce_candidates(d, h1, q)
    for t in range(1, max_tries + 1):
        k = next(gen)
        if 0 < k < q:
            return k, t
    return None, max_tries


def der_int(v):
    b = v.to_bytes((v.bit_length() + 7) // 8 or 1, "big")
    if b[0] & 0x80:
        b = b"\x00" + b
    return b"\x02" + bytes([len(b)]) + b


def der_sig(r, s):
    body = der_int(r) + der_int(s)
    return b"\x30" + bytes([len(body)]) + body


def sign_rs(c, d, msg, max_tries=MAX_TRIES):
    """(r, s, k) or None when max_tries candidates were all rejected."""
    h1 = hashlib.sha256(msg).digest()
    e = int.from_bytes(h1, "big") % c.n
    gen = nonce_candidates(d, h1, c.n)
    for _ in range(max_tries):
        k = next(gen)
        if not 0 < k < c.n:
            continue
        r = mul(c, k, c.G)[0] % c.n
        s = pow(k, -1, c.n) * (e + d * r) % c.n
        if r and s:
            return r, s, k
    return None


def sign(c, d, msg):
    """The DER signature (bytes), or None on exhaustion (CORDAHIP_SIGN_FAILED)."""
    rs = sign_rs(c, d, msg)
    return None if rs is None else der_sig(rs[0], rs[1])


def verify(c, pub, msg, r, s):
    if not (0 < r < c.n and 0 < s < c.n):
        return False
    e = int.from_bytes(hashlib.sha256(msg).digest(), "big") % c.n
    w = pow(s, -1, c.n)
    Q = (int.from_bytes(pub[1:33], "big"), int.from_bytes(pub[33:65], "big"))
    P = add(c, mul(c, e * w % c.n, c.G), mul(c, r * w % c.n, Q))
    return P is not None and P[0] % c.n == r


# ---- the kernel's scalar multiplication, step for step ----------------------------
def split_min(k, n):
    """(k', flipped) with k' = min(k, n - k)."""
    t = n - k
    return (t, 1) if t < k else (k, 0)


def recode(kp):
    """Digits d_j in [-7, 8], j = 0..63, with sum d_j 16^j = kp; and the carry out."""
    d, carry = [], 0
    for j in range(64):
        v = ((kp >> (4 * j)) & 15) + carry
        carry = 1 if v > 8 else 0
        d.append(v - 16 * carry)
    return d, carry


class ExceptionalAddition(AssertionError):
    pass


def general_add(c, P, Q):
    """The chord formula alone: what the branch-free addition computes when both flags are clear."""
    if P[0] == Q[0]:
        raise ExceptionalAddition("accumulator equals the entry or its inverse")
    return add(c, P, Q)


_TABLES = {}


def comb_table(c):
    """{(j, d): [d 16^j]G}, d = 1..8, j = 0..63 -- the kernel's comb table, affine."""
    if c.scheme not in _TABLES:
        t, P = {}, c.G
        for j in range(64):
            E = None
            for d in range(1, 9):
                E = add(c, E, P)
                t[(j, d)] = E
            for _ in range(4):
                P = add(c, P, P)
        _TABLES[c.scheme] = t
    return _TABLES[c.scheme]


def comb_mult(c, kp, table=None):
    """[kp]G as the kernel does it: digits from the top; at each position the sum is selected among
    {accumulator, entry, general sum} by the flags (accumulator at infinity, digit zero).
    Returns (point, trace) with trace[j] in {'keep', 'lift', 'sum'}."""
    digits, carry = recode(kp)
    assert carry == 0
    acc, trace = None, {}
    for j in range(63, -1, -1):
        dj = digits[j]
        if dj == 0:
            trace[j] = "keep"
            continue
        E = (table or comb_table(c))[(j, abs(dj))]
        if dj < 0:
            E = neg(c, E)
        if acc is None:
            acc, trace[j] = E, "lift"
        else:
            acc, trace[j] = general_add(c, acc, E), "sum"
    return acc, trace


def sign_like_kernel(c, d, msg):
    """The signature computed the kernel's way (split, recode, comb); equals sign()."""
    h1 = hashlib.sha256(msg).digest()
    e = int.from_bytes(h1, "big") % c.n
    gen = nonce_candidates(d, h1, c.n)
    for _ in range(MAX_TRIES):
        k = next(gen)
        if not 0 < k < c.n:
            continue
        kp, flip = split_min(k, c.n)
        P, _ = comb_mult(c, kp)
        r = P[0] % c.n
        kinv = pow(kp, -1, c.n)
        if flip:
            kinv = c.n - kinv
        s = kinv * (e + d * r) % c.n
        if r and s:
            return der_sig(r, s)
    return None
