"""The generic ECDSA verifier's ladder (K2: ecdsa_prep_lane / ecdsa_ladder_lane, corda_amd/csrc/ecdsa.hip)
on lanes built to take the exceptional branches of its point additions: the accumulator equal to a
G-table entry (jmadd falls into jdbl), equal to an entry's inverse (infinity in the middle of the
ladder, doublings of infinity, a restart from it), a sum that ends at infinity (x_check answers
BAD_SIG), Booth digits at the table ends and chosen scalars for the sign handling and secp256k1's GLV
recombination. The lanes are tests/golden/ecdsa_ladder_vectors.json
(tests/golden/make_ecdsa_ladder_vectors.py; tests/test_ec_ladder_model.py checks the events it records).
Every status is compared with the C oracle lane by lane and with the fixture."""
import json
import os

import numpy as np
import pytest

from corda_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_SIG = _lib.OK, 1
PAD = 100
A5_WORD = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def ladder_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "ecdsa_ladder_vectors.json")) as f:
        vs = json.load(f)["vectors"]
    vs = [dict(v, pub=bytes.fromhex(v["pub"]), sig=bytes.fromhex(v["sig"]), msg=bytes.fromhex(v["msg"])) for v in vs]
    # interleaved by curve, so that every wave holds both
    by = {s: [v for v in vs if v["scheme"] == s] for s in (2, 3)}
    out = []
    for i in range(max(len(x) for x in by.values())):
        out += [by[s][i] for s in (2, 3) if i < len(by[s])]
    assert len(out) == len(vs) >= 100 and {v["status"] for v in out} == {OK, BAD_SIG}
    return out


def lanes_of(vs):
    return [(v["scheme"], v["pub"], v["sig"], v["msg"]) for v in vs]


def oracle_batch(oracle, lanes):
    n = len(lanes)
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)  # noqa: E731
    buf = lambda xs: np.frombuffer(b"".join(xs) or b"\0", np.uint8).copy()  # noqa: E731
    sc = np.asarray([x[0] for x in lanes], np.uint8)
    pubs, sigs, msgs = [x[1] for x in lanes], [x[2] for x in lanes], [x[3] for x in lanes]
    kb, ko, sb, so, mb, mo = buf(pubs), off(pubs), buf(sigs), off(sigs), buf(msgs), off(msgs)
    want = np.zeros(n, np.uint8)
    oracle.oracle_ecdsa_verify_batch(n, sc.ctypes.data, kb.ctypes.data, ko.ctypes.data, sb.ctypes.data, so.ctypes.data,
                                     mb.ctypes.data, mo.ctypes.data, want.ctypes.data, 8)
    return want


def verdict_bits(words, n):
    return np.array([(int(words[i >> 6]) >> (i & 63)) & 1 for i in range(n)], np.uint8)


def compress(pub):
    return bytes([2 + (pub[64] & 1)]) + pub[1:33]


def host_batch(eng, lanes, want, what):
    st, vd = eng.verify_batch([x[0] for x in lanes], [x[1] for x in lanes], [x[2] for x in lanes], [x[3] for x in lanes])
    bad = np.nonzero(st != want)[0]
    assert not len(bad), (what, [(int(i), lanes[i][0], int(st[i]), int(want[i])) for i in bad[:10]])
    words = (len(lanes) + 63) // 64
    bits = verdict_bits(vd, words * 64)
    assert np.array_equal(bits[:len(lanes)], (want == OK).astype(np.uint8)) and not bits[len(lanes):].any(), what


def dense_call(eng, lanes):
    """cordahip_ecdsa_verify_device, outputs 0xA5 between guards; every third key compressed."""
    import torch
    dev = torch.device("cuda:0")
    n = len(lanes)
    words = (n + 63) // 64
    keys = [compress(x[1]) if i % 3 == 0 else x[1] for i, x in enumerate(lanes)]
    K, S = np.zeros((n, 65), np.uint8), np.zeros((n, 72), np.uint8)
    for i, (_, _, sig, msg) in enumerate(lanes):
        assert len(sig) <= 72 and len(msg) == 32
        K[i, :len(keys[i])] = np.frombuffer(keys[i], np.uint8)
        S[i, :len(sig)] = np.frombuffer(sig, np.uint8)
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8)).to(dev)  # noqa: E731
    t_st = torch.full((PAD + n + PAD,), 0xA5, dtype=torch.uint8, device=dev)
    t_vd = torch.full((2 + words + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
    eng.ecdsa_verify_device(up([x[0] for x in lanes]), up(K), up([len(k) for k in keys]), up(S),
                            up([len(x[2]) for x in lanes]),
                            up(np.frombuffer(b"".join(x[3] for x in lanes), np.uint8).reshape(n, 32)),
                            t_st[PAD:PAD + n], t_vd[2:2 + words], stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    st_all, vd_all = t_st.cpu().numpy(), t_vd.cpu().numpy().view(np.uint64)
    assert (st_all[:PAD] == 0xA5).all() and (st_all[PAD + n:] == 0xA5).all()
    assert (vd_all[:2] == A5_WORD).all() and (vd_all[2 + words:] == A5_WORD).all()
    got = st_all[PAD:PAD + n].copy()
    bits = verdict_bits(vd_all[2:2 + words], words * 64)
    assert np.array_equal(bits[:n], (got == OK).astype(np.uint8)) and not bits[n:].any()
    return got


def report(vs, got, want):
    return [(v["scheme"], v["for"], int(g), int(w)) for v, g, w in zip(vs, got, want) if g != w][:10]


def test_generic_host_batch(engine, oracle, ladder_vectors, ec_vectors):
    vs = ladder_vectors
    lanes = lanes_of(vs)
    want = oracle_batch(oracle, lanes)
    assert want.tolist() == [v["status"] for v in vs], report(vs, want, [v["status"] for v in vs])
    host_batch(engine, lanes, want, "all")
    # partial and mixed-curve waves, and runs of the batched inversion next to lanes decided before it:
    # each length takes its special lanes from another place in the fixture and pads with goldens
    pos = 0
    for n in (1, 63, 65, 257):
        take = max(1, 2 * n // 3)
        special = [vs[(pos + i) % len(vs)] for i in range(take)]
        start = 7 * n % 500
        gold = ec_vectors[start:start + n - take]
        assert len(gold) == n - take
        pos += take
        mixed = []
        for i in range(n):  # two fixture lanes, one golden, ...
            from_fixture = (i % 3 != 2 and special) or not gold
            mixed.append((special if from_fixture else gold).pop(0))
        ml = lanes_of(mixed)
        mw = oracle_batch(oracle, ml)
        assert mw.tolist() == [v["status"] for v in mixed]
        assert sum("for" in v for v in mixed) == take
        host_batch(engine, ml, mw, n)


def test_dense_device_call(engine, oracle, ladder_vectors):
    vs = ladder_vectors
    lanes = lanes_of(vs)
    want = oracle_batch(oracle, lanes)
    got = dense_call(engine, lanes)
    assert np.array_equal(got, want), report(vs, got, want)
    assert got.tolist() == [v["status"] for v in vs]


def test_routed_generic_instances(oracle, ladder_vectors):
    """Routing on with one unrelated key registered per curve: every fixture lane goes through
    ecdsa_prep_idx_kernel / ecdsa_ladder_idx_kernel, none to the keyed verifier."""
    import bc_ecdsa as bc
    from corda_amd.engine import Engine
    vs = ladder_vectors
    lanes = lanes_of(vs)
    want = oracle_batch(oracle, lanes)
    with Engine(1) as eng:
        for scheme in (2, 3):
            key = bc.keypair(scheme, 0xC0FFEE + scheme)
            assert all(x[1] != key for x in lanes)
            kid, st = eng.vkey_add_ecdsa(scheme, key)
            assert st == OK
        eng.vkey_set_routing_ecdsa(True)
        before = eng.vkey_route_stats_ecdsa()
        got = dense_call(eng, lanes)
        after = eng.vkey_route_stats_ecdsa()
        assert (after[0] - before[0], after[1] - before[1]) == (0, len(lanes))
        assert np.array_equal(got, want), report(vs, got, want)
        assert got.tolist() == [v["status"] for v in vs]
        before = after
        host_batch(eng, lanes, want, "routed host batch")
        after = eng.vkey_route_stats_ecdsa()
        assert (after[0] - before[0], after[1] - before[1]) == (0, len(lanes))


def test_twins_reject(engine, oracle, ladder_vectors):
    """The first message bit flipped on every valid lane: the same keys and signatures next to the same
    branches, all BAD_SIG."""
    vs = [v for v in ladder_vectors if v["status"] == OK]
    lanes = [(v["scheme"], v["pub"], v["sig"], bytes([v["msg"][0] ^ 0x80]) + v["msg"][1:]) for v in vs]
    want = oracle_batch(oracle, lanes)
    assert (want == BAD_SIG).all()
    host_batch(engine, lanes, want, "twins")
    got = dense_call(engine, lanes)
    assert np.array_equal(got, want), report(vs, got, want)
