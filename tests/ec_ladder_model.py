"""CPU model of the generic ECDSA verifier's ladder schedule (K2: ecdsa_ladder_lane in
corda_amd/csrc/ecdsa.hip), shared by tests/test_ec_ladder_model.py, tests/test_gpu_ecdsa_ladder.py
and tests/golden/make_ecdsa_ladder_vectors.py. Not a test module.

The Booth recoding of sc25519.hpp (booth_digit<W>), the sign split and secp256k1's GLV split (the
latter two from tools/gen_fp29_consts.py, which states the kernel's split step for step), and the
exact order of the ladder's doublings and additions: P-256 runs 64 windows of 4 bits over u2 with a
20-bit digit of u1 every fifth window; secp256k1 runs 33 windows over the four GLV halves, [d1]Q,
phi([d2]Q), then every fifth window the digits of the G and lambda-G tables. `scalar_trace` follows
the accumulator as a scalar mod n for a key Q = [dq]G and records where the additions meet their
exceptional branches (the accumulator equal to the addend, equal to its inverse, at infinity) and
the digits at the table ends; `trace` runs the same schedule on affine points and must see the same
events."""
import hashlib
import os
import sys

import bc_ecdsa as bc
import ec_vkey_model as vk

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_fp29_consts as gen  # noqa: E402

K1, R1 = 2, 3
Q_BITS = 4
G_BITS = 20                     # ecdsa.hip: EC_G_BITS
G_EVERY = G_BITS // Q_BITS      # a G digit every fifth window
Q_MAX, G_MAX = 1 << (Q_BITS - 1), 1 << (G_BITS - 1)
WINDOWS = {R1: 64, K1: 33}      # 4-bit windows: 256 bits, and 132 bits for halves below 2^129
LAMBDA, BETA = gen.LAMBDA, gen.BETA
TABLES = {R1: ("Q", "G"), K1: ("Q", "PQ", "G", "LG")}
assert bc.CURVES[K1].n == gen.N_K1 and bc.CURVES[R1].n == gen.N_R1


def booth(u: int, W: int, j: int) -> int:
    """sc25519.hpp booth_digit<W>(k, j): bits Wj-1 .. Wj+W-1 of a scalar below 2^256 (bit -1 and the
    bits from 256 up are zero), digit in [-2^(W-1), 2^(W-1)]."""
    assert 0 <= u < 1 << 256
    v = ((u << 1) >> (W * j)) & ((1 << (W + 1)) - 1)
    return ((v + 1) >> 1) - ((v >> W) << W)


def split_sign(u: int, n: int):
    """ecdsa.hip split_sign: (magnitude, negative); negative when bit 255 is set."""
    return gen.signed_mag(u, n)


def glv_split(u: int):
    """ecdsa.hip glv_split: u == r1 + r2 lambda (mod n), both as residues mod n."""
    return gen.glv_split(u)


def halves(scheme, u1, u2):
    """The ladder's scalar halves: table -> (magnitude, negative)."""
    n = bc.CURVES[scheme].n
    assert 0 <= u1 < n and 0 <= u2 < n
    if scheme == K1:
        a1, a2 = glv_split(u1)
        b1, b2 = glv_split(u2)
        h = {"G": split_sign(a1, n), "LG": split_sign(a2, n), "Q": split_sign(b1, n), "PQ": split_sign(b2, n)}
        assert all(m < 1 << 129 for m, _ in h.values())
    else:
        h = {"G": split_sign(u1, n), "Q": split_sign(u2, n)}
        assert all(m < 1 << 255 for m, _ in h.values())
    return h


def additions(scheme, u1, u2):
    """ecdsa_ladder_lane's operations in order: ("dbl4", window, None, 0) for a window's four
    doublings and ("add", window, table, m) for an addition of [|m|] of the table's base point, m the
    Booth digit with its half's sign applied (the sign of m is the sign of the added point). Zero
    digits add nothing, as in the kernel."""
    h = halves(scheme, u1, u2)
    top = WINDOWS[scheme] - 1
    qt = [t for t in TABLES[scheme] if t in ("Q", "PQ")]
    gt = [t for t in TABLES[scheme] if t in ("G", "LG")]
    ops = []
    for j in range(top, -1, -1):
        if j != top:
            ops.append(("dbl4", j, None, 0))
        for t in qt:
            d = booth(h[t][0], Q_BITS, j)
            if d:
                ops.append(("add", j, t, -d if h[t][1] else d))
        if j % G_EVERY == 0:
            for t in gt:
                d = booth(h[t][0], G_BITS, j // G_EVERY)
                if d:
                    ops.append(("add", j, t, -d if h[t][1] else d))
    return ops


def _walk(ops, zero, dbl4, addend, same, opposite, plus):
    """The schedule over an abstract group: returns (accumulator, events)."""
    ev = []
    acc, started = zero, False
    for op, j, t, m in ops:
        if op == "dbl4":
            if started and acc == zero:
                ev.append(("dbl_of_inf", j, None))
            acc = dbl4(acc)
            continue
        if t in ("Q", "PQ") and abs(m) == Q_MAX:
            ev.append(("qmax", j, t))
        if t in ("G", "LG") and abs(m) == G_MAX:
            ev.append(("gmax", j, t))
        e = addend(t, m)
        if acc == zero:
            if started:
                ev.append(("from_inf", j, t))
        elif same(acc, e):
            ev.append(("dbl", j, t))
        elif opposite(acc, e):
            ev.append(("inf", j, t))
        acc = plus(acc, e)
        started = True
    if acc == zero:
        ev.append(("final_inf", 0, None))
    return acc, ev


def scalar_trace(scheme, dq, u1, u2):
    """The accumulator as a scalar mod n for the key Q = [dq]G (lambda-table terms times lambda):
    (final scalar, [(event, window, table)])."""
    n = bc.CURVES[scheme].n
    base = {"G": 1, "LG": LAMBDA, "Q": dq % n, "PQ": dq * LAMBDA % n}
    return _walk(additions(scheme, u1, u2), 0, lambda a: 16 * a % n, lambda t, m: m * base[t] % n,
                 lambda a, e: a == e, lambda a, e: (a + e) % n == 0, lambda a, e: (a + e) % n)


def mul(c, k, pt):
    """[k]pt, k >= 0, by double-and-add on ec_vkey_model.add."""
    acc = None
    for bit in bin(k)[2:]:
        acc = vk.add(c, acc, acc)
        if bit == "1":
            acc = vk.add(c, acc, pt)
    return acc


def trace(scheme, Q, u1, u2):
    """The same schedule on affine points (None: infinity): the per-lane table [1..8]Q by repeated
    addition as ecdsa_prep_lane builds it, phi(x, y) = (beta x, y), the G tables' entries by
    multiplication. Returns (point, events)."""
    c = bc.CURVES[scheme]
    qtab = [None, Q, vk.add(c, Q, Q)]
    for _ in range(3, Q_MAX + 1):
        qtab.append(vk.add(c, qtab[-1], Q))

    def addend(t, m):
        if t in ("Q", "PQ"):
            e = qtab[abs(m)]
        else:
            e = mul(c, abs(m), c.G)
        if t in ("PQ", "LG"):
            e = (e[0] * BETA % c.p, e[1])
        return vk.neg(c, e) if m < 0 else e

    def dbl4(a):
        for _ in range(4):
            a = vk.add(c, a, a)
        return a

    return _walk(additions(scheme, u1, u2), None, dbl4, addend, lambda a, e: a == e,
                 lambda a, e: a[0] == e[0] and a != e, lambda a, e: vk.add(c, a, e))


def scalars(scheme, sig: bytes, msg: bytes):
    """(r, u1, u2) of a DER signature with r, s in [1, n)."""
    n = bc.CURVES[scheme].n
    r, s = bc.der_decode(sig)
    assert 1 <= r < n and 1 <= s < n
    e = int.from_bytes(hashlib.sha256(msg).digest(), "big") % n
    w = pow(s, -1, n)
    return r, e * w % n, r * w % n


def has(events, name, table=None):
    return [x for x in events if x[0] == name and (table is None or x[2] == table)]
