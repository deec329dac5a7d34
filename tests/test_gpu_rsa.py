"""RSA_SHA256 (RSASSA-PSS) on the GPU: the cooperative modular exponentiation against
Python's pow, the golden vectors (tests/golden/rsa_pss_vectors.json, pinned by OpenSSL
through bc_rsa_pss.py) through the generic batch with CORDAHIP_FLAG_RSA_ON_DEVICE, mixed
batches, fresh CRT-signed corpora, the dense device entry point, tickets and memory."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from conftest import ROOT

import bc_rsa_pss as bc

pytestmark = pytest.mark.gpu

RSA, K1, R1, ED, SPHINCS = 1, 2, 3, 4, 5
CLASSES = (64, 96, 128)


def class_words(bits):
    return 64 if bits <= 2048 else 96 if bits <= 3072 else 128


def to_words(x, w):
    return np.frombuffer(x.to_bytes(4 * w, "little"), dtype="<u4").astype(np.uint32)


def from_words(row):
    return int.from_bytes(np.ascontiguousarray(row, dtype="<u4").tobytes(), "little")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        g = json.load(f)
    keys = [dict(k, der=bytes.fromhex(k["der"])) for k in g["keys"]]
    for k in keys:
        for name in ("n", "e", "d", "p", "q"):
            if name in k:
                k[name] = int(k[name], 16)
    vs = [dict(v, sig=bytes.fromhex(v["sig"]), msg=bytes.fromhex(v["msg"])) for v in g["vectors"]]
    return keys, vs


def signing_keys(keys):
    """the fixture's test keys the GPU path takes and that can sign (p, q, d recorded)"""
    return [k for k in keys if "d" in k and not isinstance(bc.decode_key(k["der"]), int)]


def fresh_signature(rng, k, msg, flip=False):
    em = bc.encode_em(msg, k["n"].bit_length(), rng.randbytes(32))
    s = bc.sign_crt(em, k["p"], k["q"], k["d"])
    sig = bytearray(s.to_bytes((k["n"].bit_length() + 7) // 8, "big"))
    if flip:
        sig[rng.randrange(len(sig))] ^= 1 << rng.randrange(8)
    return bytes(sig)


def adversarial_moduli(rng, w):
    r = 1 << (32 * w)
    return [r - 1, (1 << (32 * w - 1)) + 1, (rng.getrandbits(32 * w - 97) << 96) | ((1 << 96) - 1) | (1 << (32 * w - 1)),
            rng.getrandbits(32 * w) | 1 | (1 << (32 * w - 1)), rng.getrandbits(32 * w - 700) | 1,
            rng.getrandbits(32 * w - 31) | 1]


def run_public_op(engine, torch_dev, w, rows):
    torch, dev = torch_dev
    n = len(rows)
    mod = np.stack([to_words(r[0], w) for r in rows])
    exp = np.array([r[1] for r in rows], dtype=np.uint32)
    inp = np.stack([to_words(r[2], w) for r in rows])
    t = lambda a: torch.from_numpy(a.view(np.int32).copy()).to(dev)  # noqa: E731
    tm, te, ti = t(mod), t(exp), t(inp)
    out = torch.full((n, w), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    engine.rsa_public_op_device(tm, te, ti, out, stream=s)
    s.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    return [from_words(got[i]) for i in range(n)]


@pytest.mark.parametrize("w", CLASSES)
def test_public_op_matches_pow(engine, torch_dev, w):
    """Exact equality of every output row: adversarial and random moduli and operands,
    mixed exponents in adjacent groups, row counts that leave partial groups and waves."""
    from corda_amd import _lib
    t = _lib.RSA_GROUP_LANES
    rng = random.Random(0xA5A + w)
    exps = [3, 17, 65537, (1 << 32) - 1, 1]
    for n in (1, t - 1, t + 1, 64 // t + 1, 200):
        mods = adversarial_moduli(rng, w)
        rows = []
        for i in range(n):
            m = mods[i % len(mods)] if i < 48 else rng.getrandbits(rng.randrange(1024, 32 * w + 1)) | 1
            a = [m - 1, 0, 1, rng.randrange(m), rng.randrange(m)][(i // len(mods)) % 5]
            rows.append((m, exps[i % len(exps)], a))
        got = run_public_op(engine, torch_dev, w, rows)
        for i, (m, e, a) in enumerate(rows):
            assert got[i] == pow(a, e, m), (w, n, i, hex(m)[:18], e)


def test_public_op_contract_violations_give_zero_rows(engine, torch_dev):
    """An even or zero modulus, exponent 0 and in >= modulus come back as zero rows, and the
    rows beside them in the same wave are exact."""
    rng = random.Random(7)
    w = 64
    m = rng.getrandbits(2048) | 1 | (1 << 2047)
    rows = [(m, 65537, 5), (m + 1, 65537, 5), (m, 0, 5), (m, 65537, m), (m, 65537, m + 2), (0, 3, 0), (m, 3, m - 1)]
    got = run_public_op(engine, torch_dev, w, rows)
    want = [pow(5, 65537, m), 0, 0, 0, 0, 0, pow(m - 1, 3, m)]
    assert got == want


def batch_of(keys, vs):
    return ([RSA] * len(vs), [keys[v["key"]]["der"] for v in vs], [v["sig"] for v in vs], [v["msg"] for v in vs])


def verdict_bits(verdict, n):
    return [(int(verdict[i // 64]) >> (i % 64)) & 1 for i in range(n)]


@pytest.mark.parametrize("is_valid", (False, True))
def test_golden_vectors_generic_batch(engine, golden, is_valid):
    keys, vs = golden
    st, verdict = engine.verify_batch(*batch_of(keys, vs), is_valid=is_valid, rsa=True)
    name = "status_is_valid" if is_valid else "status"
    bad = [(i, v["cat"], keys[v["key"]]["name"], int(s), v[name]) for i, (v, s) in enumerate(zip(vs, st))
           if int(s) != v[name]]
    assert not bad, bad[:20]
    assert verdict_bits(verdict, len(vs)) == [int(v[name] == bc.OK) for v in vs]
    assert sum(v["cat"] == "top_bit" and v[name] == bc.OK for v in vs) >= 5  # the BC-lenient rule is exercised


def test_flag_off_is_unsupported_and_flag_is_accepted(engine, golden):
    from corda_amd import _lib
    from corda_amd._lib import SigBatch, lib
    keys, vs = golden
    for is_valid in (False, True):
        st, verdict = engine.verify_batch(*batch_of(keys, vs), is_valid=is_valid)
        assert [int(s) for s in st] == [bc.UNSUPPORTED] * len(vs)
        assert not any(verdict_bits(verdict, len(vs)))
    # the flag's value through the C-ABI: 2 is a valid flags word (INVALID_ARG without the feature), 4 is not
    v = vs[0]
    arrs = engine._csr([keys[v["key"]]["der"]]), engine._csr([v["sig"]]), engine._csr([v["msg"]])
    sch = np.array([RSA], np.uint8)
    for flags, rc, want in ((2, 0, bc.OK), (3, 0, bc.OK), (4, -1, 0xEE), (0, 0, bc.UNSUPPORTED)):
        status = np.full(1, 0xEE, np.uint8)
        (kb, ko), (sb, so), (mb, mo) = arrs
        b = SigBatch(1, sch.ctypes.data, kb.ctypes.data, ko.ctypes.data, sb.ctypes.data, so.ctypes.data,
                     mb.ctypes.data, mo.ctypes.data, status.ctypes.data, None, flags, kb.size, sb.size, mb.size)
        assert lib().cordahip_sig_verify(engine.ctx, ctypes.byref(b)) == rc, flags
        assert int(status[0]) == want, flags
    assert _lib.FLAG_RSA_ON_DEVICE == 2
    assert "#define CORDAHIP_FLAG_RSA_ON_DEVICE 2u" in open(os.path.join(ROOT, "include", "cordahip.h")).read()


def test_mixed_batch_in_input_order(engine, golden, ec_vectors, ed_vectors):
    """200 ECDSA, 200 Ed25519 and ~150 RSA lanes of all three classes, interleaved, with
    scheme-5 lanes and malformed keys: statuses in input order, verdict words = (status == OK)."""
    keys, vs = golden
    rng = random.Random(99)
    rare = ("malformed_key", "malformed_key_empty", "declined_key", "declined_key_valid", "top_bit", "m_above_em",
            "stripped_leading_zero", "wrong_key", "salt_len_0")
    rsa_vs = [v for v in vs if v["cat"] in rare] + [v for v in vs if v["cat"] not in rare + ("s_edge",)][:95]
    rsa_vs += [v for v in vs if v["cat"] == "s_edge"][:20]
    assert 140 <= len(rsa_vs) <= 160
    assert {class_words(keys[v["key"]]["n"].bit_length()) for v in rsa_vs if "n" in keys[v["key"]]} >= set(CLASSES)
    lanes = [(v["scheme"], v["pub"], v["sig"], v["msg"], v["status"]) for v in ec_vectors[:200]]
    lanes += [(ED, v["pub"], v["sig"], v["msg"], v["status"]) for v in ed_vectors[:200]]
    lanes += [(RSA, keys[v["key"]]["der"], v["sig"], v["msg"], v["status"]) for v in rsa_vs]
    lanes += [(SPHINCS, b"\x01" * 32, b"\x02" * 64, b"m", bc.UNSUPPORTED)] * 7
    rng.shuffle(lanes)
    st, verdict = engine.verify_batch([l[0] for l in lanes], [l[1] for l in lanes], [l[2] for l in lanes],
                                      [l[3] for l in lanes], rsa=True)
    want = [l[4] for l in lanes]
    bad = [(i, lanes[i][0], int(s), w) for i, (s, w) in enumerate(zip(st, want)) if int(s) != w]
    assert not bad, bad[:20]
    assert verdict_bits(verdict, len(lanes)) == [int(w == 0) for w in want]
    assert sum(1 for l in lanes if l[0] == RSA and l[4] == bc.BAD_KEY) >= 5


def test_random_corpus(engine, golden):
    """240 fresh CRT-signed lanes over the fixture's keys, every fifth signature bit-flipped."""
    keys, _ = golden
    ks = signing_keys(keys)
    assert len(ks) >= 10
    rng = random.Random(0xC0DA)
    ders, sigs, msgs, want = [], [], [], []
    for i in range(240):
        k = ks[i % len(ks)]
        m = rng.randbytes(rng.randrange(1, 200))
        sig = fresh_signature(rng, k, m, flip=i % 5 == 4)
        ders.append(k["der"])
        sigs.append(sig)
        msgs.append(m)
        want.append(bc.verify(k["der"], sig, m))
    st, verdict = engine.verify_batch([RSA] * 240, ders, sigs, msgs, rsa=True)
    assert [int(s) for s in st] == want
    assert sum(int(s) == bc.OK for s in st) == 240 - 48
    assert all(w == (bc.BAD_SIG if i % 5 == 4 else bc.OK) for i, w in enumerate(want))


@pytest.mark.parametrize("w", CLASSES)
def test_dense_pss_verify_device(engine, torch_dev, golden, w):
    """rsa_pss_verify_device per class with n = 1 and n = 131 on a torch stream: sig_len 0,
    k - 1, k and slot + 1, an even and a short modulus, verdict words."""
    torch, dev = torch_dev
    keys, _ = golden
    ks = [k for k in signing_keys(keys) if class_words(k["n"].bit_length()) == w]
    assert ks
    rng = random.Random(w)
    msg_len = 32
    for n in (1, 131):
        mod = np.zeros((n, w), np.uint32)
        exp = np.zeros(n, np.uint32)
        sigs = np.zeros((n, 4 * w), np.uint8)
        sl = np.zeros(n, np.uint16)
        msgs = np.zeros((n, msg_len), np.uint8)
        want = []
        for i in range(n):
            k = ks[i % len(ks)]
            kl = (k["n"].bit_length() + 7) // 8
            m = rng.randbytes(msg_len)
            sig = fresh_signature(rng, k, m)
            nn, length, st = k["n"], len(sig), bc.OK
            kind = i % 9 if n > 1 else 0
            if kind == 1:
                length, st = 0, bc.EMPTY
            elif kind == 2:  # the signature cut to k - 1 bytes: another integer
                sig, length = sig[:kl - 1], kl - 1
                st = bc.verify(k["der"], sig, m)
            elif kind == 3:
                length, st = 4 * w + 1, bc.BAD_SIG  # beyond the slot: nothing past it is read
            elif kind == 4:
                nn, st = k["n"] + 1, bc.UNSUPPORTED  # even modulus
            elif kind == 5:
                nn, st = k["n"] >> (k["n"].bit_length() - 1000) | 1, bc.UNSUPPORTED  # below 1024 bits
            elif kind == 6:
                sig = bytes([sig[0] ^ 0x01]) + sig[1:]
                st = bc.verify(k["der"], sig, m)
            mod[i] = to_words(nn, w)
            exp[i] = k["e"]
            sigs[i, :min(len(sig), 4 * w)] = np.frombuffer(sig[:4 * w], np.uint8)
            sl[i] = length
            msgs[i] = np.frombuffer(m, np.uint8)
            want.append(st)
        t = lambda a, ty: torch.from_numpy(a.view(ty).copy()).to(dev)  # noqa: E731
        tm, te, ts, tl, tg = t(mod, np.int32), t(exp, np.int32), t(sigs, np.uint8), t(sl, np.int16), t(msgs, np.uint8)
        status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
        verdict = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream())
        engine.rsa_pss_verify_device(tm, te, ts, tl, tg, status, verdict, stream=s)
        s.synchronize()
        got = [int(x) for x in status.cpu().numpy()]
        assert got == want, [(i, g, x) for i, (g, x) in enumerate(zip(got, want)) if g != x][:10]
        vd = verdict.cpu().numpy().view(np.uint64)
        assert verdict_bits(vd, n) == [int(x == bc.OK) for x in want]
        if n > 1:
            assert {bc.OK, bc.BAD_SIG, bc.EMPTY, bc.UNSUPPORTED} <= set(want)


def test_tickets_with_and_without_the_flag(engine, golden):
    """Two flagged tickets and one unflagged outstanding at once."""
    keys, vs = golden
    a, b2 = vs[:90], vs[60:]
    t1 = engine.verify_batch(*batch_of(keys, a), rsa=True, async_=True)
    t2 = engine.verify_batch(*batch_of(keys, b2), rsa=True, is_valid=True, async_=True)
    t3 = engine.verify_batch(*batch_of(keys, a), async_=True)
    st3, _ = t3.wait()
    st1, v1 = t1.wait()
    st2, v2 = t2.wait()
    assert [int(s) for s in st1] == [v["status"] for v in a]
    assert [int(s) for s in st2] == [v["status_is_valid"] for v in b2]
    assert [int(s) for s in st3] == [bc.UNSUPPORTED] * len(a)
    assert verdict_bits(v1, len(a)) == [int(v["status"] == bc.OK) for v in a]
    assert verdict_bits(v2, len(b2)) == [int(v["status_is_valid"] == bc.OK) for v in b2]


def test_memory_accounting(golden):
    """An RSA call grows in_use, cordahip_trim returns it; a context that never sets the flag
    holds exactly what it holds for the same calls without any RSA lane's buffers."""
    from corda_amd.engine import Engine
    keys, vs = golden
    lanes = batch_of(keys, vs[:64])
    with Engine(1) as e:
        e.verify_batch(*lanes)  # flag off: the generic pipeline's own buffers
        e.trim()
        base = e.device_mem(0)[0]
        e.verify_batch(*lanes)
        off = e.device_mem(0)[0]
        e.trim()
        assert e.device_mem(0)[0] == base
        e.verify_batch(*lanes, rsa=True)
        on = e.device_mem(0)[0]
        assert on > off >= base  # the RSA stage and workspace are accounted
        e.trim()
        assert e.device_mem(0)[0] == base
        e.verify_batch(*lanes)
        assert e.device_mem(0)[0] == off  # and nothing of them is left for a call without the flag
