"""CPU model of the generic ECDSA verifier's ladder (tests/ec_ladder_model.py) and the fixture built
with it (tests/golden/ecdsa_ladder_vectors.json): the Booth recoding sums back to the scalar inside
the digit bounds, the GLV halves recombine, the schedule's sum is u1 + d u2 in the scalar domain and
[u1]G + [u2]Q on points, the model's G window is the kernel's, every vector's recorded events are
what the model derives again, and the fixture holds the lanes it was made for, per curve."""
import collections
import hashlib
import json
import os
import re

import bc_ecdsa as bc
import ec_ladder_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1, R1 = model.K1, model.R1


def _h(tag, i):
    return int.from_bytes(hashlib.sha256(b"ladder-model-%s-%d" % (tag, i)).digest(), "big")


def _edge_scalars(n):
    g = model.gen
    out = [1, n - 1, (1 << 255) - 1, 1 << 255, (1 << 255) + 1, int.from_bytes(b"\x80" * 32, "big") % n,
           int.from_bytes(b"\x81" * 32, "big") % n, int.from_bytes(b"\xff" * 32, "big") % n,
           int.from_bytes(b"\x88" * 32, "big") % n, int.from_bytes(b"\x77" * 32, "big"), 1 << 240, (1 << 20) - 1,
           1 << 19, (1 << 19) - 1, 8, 7, 0]
    if n == g.N_K1:
        out += [g.LAMBDA, n - g.LAMBDA, g.A1, g.A2, n - g.A1, 1 << 128, (1 << 128) - 1]
    return out + [_h(b"rand", i) % n for i in range(300)]


def _vectors():
    with open(os.path.join(ROOT, "tests", "golden", "ecdsa_ladder_vectors.json")) as f:
        return json.load(f)["vectors"]


def test_g_window_is_the_kernels():
    with open(os.path.join(ROOT, "corda_amd", "csrc", "ecdsa.hip")) as f:
        m = re.search(r"^#define EC_G_BITS (\d+)$", f.read(), re.M)
    assert m and int(m.group(1)) == model.G_BITS and model.G_BITS % model.Q_BITS == 0


def test_recoding_sums_to_the_scalar_within_bounds():
    for scheme, c in bc.CURVES.items():
        n = c.n
        for u in _edge_scalars(n):
            if scheme == K1:
                r1, r2 = model.glv_split(u)
                assert (r1 + r2 * model.LAMBDA - u) % n == 0
                mags = [model.split_sign(r, n) for r in (r1, r2)]
                assert all(m < 1 << 129 for m, _ in mags)
            else:
                mags = [model.split_sign(u, n)]
                assert mags[0][0] < 1 << 255
            assert all((n - m if ng else m) % n == x for (m, ng), x in zip(mags, (r1, r2) if scheme == K1 else (u,)))
            nq = model.WINDOWS[scheme]
            ng = (nq - 1) // model.G_EVERY + 1
            for m, _ in mags:
                q = [model.booth(m, model.Q_BITS, j) for j in range(nq)]
                g = [model.booth(m, model.G_BITS, j) for j in range(ng)]
                assert sum(d << (model.Q_BITS * j) for j, d in enumerate(q)) == m
                assert sum(d << (model.G_BITS * j) for j, d in enumerate(g)) == m
                assert all(abs(d) <= model.Q_MAX for d in q) and all(abs(d) <= model.G_MAX for d in g)
    # the ends of the digit ranges, by hand
    assert model.booth(8, 4, 0) == -8 and model.booth(8, 4, 1) == 1 and model.booth(0x78, 4, 1) == 8
    assert model.booth(1 << 19, 20, 0) == -(1 << 19) and model.booth(1 << 19, 20, 1) == 1
    assert model.booth(0x7ffff80000, 20, 1) == 1 << 19


def test_schedule_shape():
    """The order of operations of ecdsa_ladder_lane, on scalars whose every digit is non-zero."""
    n = bc.CURVES[R1].n
    ops = model.additions(R1, int.from_bytes(b"\x33" * 32, "big"), int.from_bytes(b"\x11" * 32, "big"))
    assert [o[0] for o in ops].count("dbl4") == 63 and ops[0] == ("add", 63, "Q", 1)
    assert [o[2] for o in ops if o[0] == "add"].count("G") == 13
    for j in range(64):
        w = [(o[0], o[2]) for o in ops if o[1] == j]
        assert w == ([("dbl4", None)] if j != 63 else []) + [("add", "Q")] + ([("add", "G")] if j % 5 == 0 else []), j
    # a negative half negates every multiplier of its table
    neg = model.additions(R1, n - int.from_bytes(b"\x33" * 32, "big"), int.from_bytes(b"\x11" * 32, "big"))
    assert [(o[0], o[1], o[2], -o[3] if o[2] == "G" else o[3]) for o in neg] == ops
    q = int.from_bytes(b"\x11" * 16, "big")
    u = (q + q * model.LAMBDA) % bc.CURVES[K1].n
    assert model.glv_split(u) == (q, q)
    ops = model.additions(K1, u, u)
    assert [o[0] for o in ops].count("dbl4") == 32 and ops[0][1] == 31  # 128-bit halves: window 32 is empty
    for j in range(32):
        w = [(o[0], o[2]) for o in ops if o[1] == j]
        assert w == [("dbl4", None), ("add", "Q"), ("add", "PQ")] + ([("add", "G"), ("add", "LG")] if j % 5 == 0 else []), j


def test_scalar_trace_ends_at_u1_plus_d_u2():
    for scheme, c in bc.CURVES.items():
        n = c.n
        for i in range(200):
            dq, u1, u2 = (_h(b"st%d" % t, i) % n for t in range(3))
            acc, ev = model.scalar_trace(scheme, dq, u1, u2)
            assert acc == (u1 + dq * u2) % n
            assert not [x for x in ev if x[0] in ("dbl", "inf", "dbl_of_inf", "from_inf", "final_inf")]
        # Q = G and u1 = u2 = 5: the key's entry meets the accumulator it equals; Q = -G: its inverse, to the end
        assert ("dbl", 0, "G") in model.scalar_trace(scheme, 1, 5, 5)[1]
        ev = model.scalar_trace(scheme, n - 1, 5, 5)[1]
        assert ev[-2:] == [("inf", 0, "G"), ("final_inf", 0, None)]


def test_point_trace_equals_multiplication():
    for scheme, c in bc.CURVES.items():
        n = c.n
        for i in range(4):
            dq, u1, u2 = (_h(b"pt%d" % t, i) % n for t in range(3))
            if i == 3:
                u1 = n - u1  # the other sign
            q = bc._mul(c, dq, c.G)
            pt, ev = model.trace(scheme, q, u1, u2)
            assert pt == bc._add(c, bc._mul(c, u1, c.G), bc._mul(c, u2, q))
            assert ev == model.scalar_trace(scheme, dq, u1, u2)[1]
        for dq in (1, n - 1):  # the exceptional branches through the point model
            pt, ev = model.trace(scheme, bc._mul(c, dq, c.G), 5, 5)
            acc, sev = model.scalar_trace(scheme, dq, 5, 5)
            assert ev == sev and pt == (bc._mul(c, acc, c.G) if acc else None)


def test_fixture_events_and_counts():
    vs = _vectors()
    assert 100 <= len(vs) <= 400
    lanes = collections.defaultdict(list)
    for v in vs:
        scheme, c = v["scheme"], bc.CURVES[v["scheme"]]
        sig, msg, d = bytes.fromhex(v["sig"]), bytes.fromhex(v["msg"]), int(v["d"], 16)
        r, u1, u2 = model.scalars(scheme, sig, msg)
        acc, ev = model.scalar_trace(scheme, d, u1, u2)
        assert [list(x) for x in ev] == v["events"], v["for"]
        assert v["status"] == (bc.BAD_SIG if acc == 0 else bc.OK)
        assert v["openssl"] == (1 if v["status"] == bc.OK else -1)
        lanes[scheme].append((v, ev, u1, u2))
    # the key bytes are [d]G: checked through the oracle on a few lanes of each curve (all of them in the generator)
    for scheme in lanes:
        for v, _, _, _ in lanes[scheme][::17]:
            assert bytes.fromhex(v["pub"]) == bc.keypair(scheme, int(v["d"], 16))
    for scheme, ls in lanes.items():
        n = bc.CURVES[scheme].n
        ok = [(v, ev) for v, ev, _, _ in ls if v["status"] == bc.OK]
        for t in ("G", "LG") if scheme == K1 else ("G",):
            assert sum(bool(model.has(ev, "dbl", t)) for _, ev in ok) >= 8, (scheme, t)
        through = [ev for _, ev in ok if all(model.has(ev, x) for x in ("inf", "dbl_of_inf", "from_inf"))]
        assert len(through) >= 8
        for ev in through:  # in this order: into infinity, doublings there, out again
            first = ev.index(model.has(ev, "inf")[0])
            assert ev[first + 1][0] == "dbl_of_inf" and model.has(ev[first + 1:], "from_inf")
        assert len({x[1] for ev in through for x in model.has(ev, "inf")}) >= 2
        ends = [ev for v, ev, _, _ in ls if v["status"] == bc.BAD_SIG]
        assert len(ends) >= 4 and all(ev[-2][0] == "inf" and ev[-1] == ("final_inf", 0, None) for ev in ends)
        for t in model.TABLES[scheme]:
            name = "qmax" if t in ("Q", "PQ") else "gmax"
            assert any(model.has(ev, name, t) for _, ev in ok), (scheme, t)
        # chosen scalars: a lane with u1 = u and one with u2 = u
        g = model.gen
        want = {"1": 1, "n-1": n - 1, "2^255-1": (1 << 255) - 1, "2^255": 1 << 255, "2^255+1": (1 << 255) + 1,
                "0x80..": int.from_bytes(b"\x80" * 32, "big") % n, "0x81..": int.from_bytes(b"\x81" * 32, "big") % n,
                "0xff..": int.from_bytes(b"\xff" * 32, "big") % n, "0x88..": int.from_bytes(b"\x88" * 32, "big") % n,
                "0x77..": int.from_bytes(b"\x77" * 32, "big"), "2^240": 1 << 240, "2^20-1": (1 << 20) - 1}
        if scheme == K1:
            want.update({"lambda": g.LAMBDA, "n-lambda": n - g.LAMBDA, "A1": g.A1, "A2": g.A2, "n-A1": n - g.A1,
                         "2^128": 1 << 128, "2^128-1": (1 << 128) - 1})
        by_for = {v["for"]: (u1, u2) for v, _, u1, u2 in ls}
        for name, u in want.items():
            assert by_for["u1 = " + name][0] == u and by_for["u2 = " + name][1] == u, (scheme, name)
        if scheme == K1:  # the longest halves the split gives, of either sign, in every position
            for which in (0, 1):
                signs = set()
                for name in ("split-max+", "split-max-"):
                    u = by_for["u%d = %s" % (which + 1, name)][which]
                    hs = [model.split_sign(r, n) for r in model.glv_split(u)]
                    assert max(m.bit_length() for m, _ in hs) == 128
                    signs.update(ng for m, ng in hs if m.bit_length() == 128)
                assert signs == {False, True}
