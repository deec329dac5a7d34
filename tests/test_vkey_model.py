"""CPU model of the keyed Ed25519 verifier (K12, corda_amd/csrc/ed25519_vkey.hip) over the
oracle's point arithmetic (oracle/i2p_ed25519.py, imported as it is): the window table
[d 256^j](-A), d = 0..128, j = 0..31, built as the registration kernel builds it (and the
same table of +B), and the lane's equation
encode(sum_j sign(e_j) tableB[j][|e_j|] + sum_j sign(d_j) table[j][|d_j|]) == R with the
signed 8-bit digits e_j of S_eff and d_j of h (ed25519_vkey.hpp). For an ordinary key, a
small-order key and a mixed-order key of tests/golden/ed25519_vectors.json it must reproduce
the oracle's accept / reject on every golden vector of that key: negative digits, zero
digits and (for the torsion keys) identity and repeated entries included."""
import collections
import hashlib

import pytest

import i2p_ed25519 as ed

DIGITS, ENTRIES = 32, 128


def point_table(base):
    """table[j][d] = [d 256^j]base in extended coordinates, d = 0..128 (entry 0: the identity)."""
    table = []
    for _ in range(DIGITS):
        row = [ed.IDENTITY]
        for _ in range(ENTRIES):
            row.append(ed.pt_add(row[-1], base))
        table.append(row)
        for _ in range(8):
            base = ed.pt_dbl(base)
    return table


def window_table(pub: bytes):
    """The key's table [d 256^j](-A) and its canonical Abyte."""
    a = ed.decode_i2p(pub)
    assert a is not None
    return point_table(ed.pt_neg(a)), ed.encode(a)


B_TABLE = point_table(ed.B_POINT)


def table_sum(p, table, k: int):
    for j, d in enumerate(digits(k)):
        e = table[j][abs(d)]
        p = ed.pt_add(p, ed.pt_neg(e) if d < 0 else e)
    return p


def digits(h: int):
    """ed25519_vkey.hpp: byte j of h + 0x7f7f..7f, minus 127."""
    t = h + int.from_bytes(b"\x7f" * 32, "little")
    assert t < 1 << 256
    d = [((t >> (8 * j)) & 0xff) - 127 for j in range(DIGITS)]
    assert sum(x << (8 * j) for j, x in enumerate(d)) == h and all(-127 <= x <= 128 for x in d)
    return d


def model_status(table, abyte: bytes, sig: bytes, msg: bytes, is_valid: bool = False) -> int:
    if not is_valid and (len(sig) == 0 or len(msg) == 0):
        return ed.EMPTY
    if len(sig) != 64:
        return ed.MALFORMED_SIG
    h = int.from_bytes(hashlib.sha512(sig[:32] + abyte + msg).digest(), "little") % ed.L
    s_eff = ed.slide_value(sig[32:]) % ed.L  # S, or S - 2^256 when slide() drops its carry
    p = table_sum(table_sum(ed.IDENTITY, B_TABLE, s_eff), table, h)
    return ed.OK if ed.encode(p) == sig[:32] else ed.BAD_SIG


def key_with_most_vectors(ed_vectors, cats):
    c = collections.Counter(v["pub"] for v in ed_vectors if v["cat"] in cats and ed.decode_i2p(v["pub"]) is not None)
    return c.most_common(1)[0][0]


@pytest.fixture(scope="module")
def keys(ed_vectors):
    return {"ordinary": key_with_most_vectors(ed_vectors, ("fixed_key", "valid", "s_plus_kL")),
            "small_order": key_with_most_vectors(ed_vectors, ("key_small_order", "key_identity_signbit")),
            "mixed_order": key_with_most_vectors(ed_vectors, ("key_mixed_order",))}


def order_divides(pub: bytes, k: int) -> bool:
    return ed.encode(ed.scalar_mult(k, ed.decode_i2p(pub))) == ed.encode(ed.IDENTITY)


def test_the_three_keys_are_what_they_are_called(keys):
    assert order_divides(keys["ordinary"], ed.L) and not order_divides(keys["ordinary"], 8)
    assert order_divides(keys["small_order"], 8)
    assert not order_divides(keys["mixed_order"], ed.L) and not order_divides(keys["mixed_order"], 8)
    assert order_divides(keys["mixed_order"], 8 * ed.L)


@pytest.mark.parametrize("kind", ["ordinary", "small_order", "mixed_order"])
def test_model_matches_oracle_on_golden_vectors(ed_vectors, keys, kind):
    pub = keys[kind]
    table, abyte = window_table(pub)
    if kind == "small_order":  # a table of a point of order <= 8: entries repeat, some are the identity
        enc = {ed.encode(e) for row in table for e in row[1:]}
        assert len(enc) <= 8 and ed.encode(ed.IDENTITY) in enc
    vecs = [v for v in ed_vectors if v["pub"] == pub]
    assert vecs
    seen = collections.Counter()
    for v in vecs:
        for is_valid in (False, True):
            want = ed.verify_status(pub, v["sig"], v["msg"], is_valid=is_valid)
            if not is_valid:
                assert want == v["status"], v["cat"]
            got = model_status(table, abyte, v["sig"], v["msg"], is_valid=is_valid)
            assert got == want, (v["cat"], v["note"], is_valid)
        seen[v["status"]] += 1
    # an accepted lane pins the whole sum; the torsion keys must have some
    if kind != "small_order" or any(v["status"] == ed.OK for v in vecs):
        assert seen[ed.OK] > 0, seen
    assert sum(seen.values()) == len(vecs)


def test_base_table_sum_is_the_scalar_multiple():
    for k in (0, 1, ed.L - 1, 1 << 252, int.from_bytes(hashlib.sha512(b"vkey-model").digest(), "little") % ed.L):
        assert ed.encode(table_sum(ed.IDENTITY, B_TABLE, k)) == ed.encode(ed.scalar_mult(k))


def test_digits_cover_the_range():
    d = digits(int.from_bytes(bytes([0x80, 0x81, 0x00, 0x7f]) + bytes(28), "little"))
    assert d[:5] == [128, -127, 1, 127, 0]
