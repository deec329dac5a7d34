"""RSA_SHA256 verification against registered public keys on the GPU (K18): the keyed modular
exponentiation against Python's pow on adversarial moduli, the golden vectors
(tests/golden/rsa_pss_vectors.json) through cordahip_rsa_verify_keyed under both flags values,
keyed against generic on fresh CRT-signed lanes, the host call in three chunks and in two launches,
the device call per width class, the registry across the three families, tickets and memory."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from conftest import ROOT

import bc_rsa_pss as bc

pytestmark = pytest.mark.gpu

RSA = 1
CLASSES = (64, 96, 128)
EXPONENTS = (3, 17, 65537, (1 << 32) - 1)
UNKNOWN, NO_ID = 16, 0xFFFFFFFF


def class_words(bits):
    return 64 if bits <= 2048 else 96 if bits <= 3072 else 128


def to_words(x, w):
    return np.frombuffer(x.to_bytes(4 * w, "little"), dtype="<u4").astype(np.uint32)


def from_words(row):
    return int.from_bytes(np.ascontiguousarray(row, dtype="<u4").tobytes(), "little")


def verdict_bits(verdict, n):
    return [(int(verdict[i // 64]) >> (i % 64)) & 1 for i in range(n)]


def adversarial_moduli(rng, w):
    """the set of test_gpu_rsa.py::adversarial_moduli"""
    r = 1 << (32 * w)
    return [r - 1, (1 << (32 * w - 1)) + 1, (rng.getrandbits(32 * w - 97) << 96) | ((1 << 96) - 1) | (1 << (32 * w - 1)),
            rng.getrandbits(32 * w) | 1 | (1 << (32 * w - 1)), rng.getrandbits(32 * w - 700) | 1,
            rng.getrandbits(32 * w - 31) | 1]


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


@pytest.fixture(scope="module")
def eng():
    """a context of this module's own: the registry holds 64 keys for all three families"""
    from corda_amd.engine import Engine
    with Engine(1) as e:
        yield e


@pytest.fixture(scope="module")
def reg(eng, golden):
    """the fixture's 11 keys that decode, registered for the module: key index -> id"""
    keys, _ = golden
    ids = {}
    for i, k in enumerate(keys):
        if not isinstance(bc.decode_key(k["der"]), int):
            kid, st = eng.vkey_add_rsa(k["der"])
            assert st == bc.OK and kid != NO_ID
            ids[i] = kid
    assert len(ids) == 11 and len(set(ids.values())) == 11
    return ids


def fresh_signature(rng, k, msg, flip=False):
    em = bc.encode_em(msg, k["n"].bit_length(), rng.randbytes(32))
    s = bc.sign_crt(em, k["p"], k["q"], k["d"])
    sig = bytearray(s.to_bytes((k["n"].bit_length() + 7) // 8, "big"))
    if flip:
        sig[rng.randrange(len(sig))] ^= 1 << rng.randrange(8)
    return bytes(sig)


def other_family_ids(e, ed_vectors, ec_vectors):
    """a live Ed25519 id and a live ECDSA id of context e"""
    ed = next(v for v in ed_vectors if v["status"] == bc.OK)
    ec = next(v for v in ec_vectors if v["status"] == bc.OK and len(v["pub"]) in (33, 65))
    ed_id, st1 = e.vkey_add_ed25519(ed["pub"])
    ec_id, st2 = e.vkey_add_ecdsa(ec["scheme"], ec["pub"])
    assert st1 == bc.OK and st2 == bc.OK
    return (ed_id, ed), (ec_id, ec)


# ---- 1. the raw op against pow ------------------------------------------------------------------
def run_public_op_keyed(e, torch_dev, w, ids, ins):
    torch, dev = torch_dev
    n = len(ids)
    t = lambda a: torch.from_numpy(a.view(np.int32).copy()).to(dev)  # noqa: E731
    ti = t(np.stack([to_words(x, w) for x in ins]))
    tk = t(np.array(ids, dtype=np.uint32))
    out = torch.full((n, w), -1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    e.rsa_public_op_keyed_device(tk, ti, out, stream=s)
    s.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    return [from_words(got[i]) for i in range(n)]


@pytest.mark.parametrize("w", CLASSES)
def test_public_op_keyed_matches_pow(eng, torch_dev, w):
    """Exact equality of every output row: 8 registered keys of the class (the adversarial moduli, a
    1024-bit modulus in the 2048-bit class, all four exponents), row counts that leave a partial group
    set, a partial wave and a second block, different keys and exponents in adjacent groups; zero rows
    for in == n, in > n, an unknown, a removed and another class's id, exact rows beside them."""
    rng = random.Random(0xB18 + w)
    mods = adversarial_moduli(rng, w)
    mods.append(rng.getrandbits(1024) | 1 | (1 << 1023) if w == 64 else rng.getrandbits(32 * w - 300) | 1)
    mods.append(rng.getrandbits(32 * w - 1) | 1 | (1 << (32 * w - 2)))
    keys = []
    for i, m in enumerate(mods):
        ex = EXPONENTS[i % 4] if i < 4 else EXPONENTS[(i + 1) % 4]  # every modulus kind meets 65537 or 2^32 - 1 somewhere
        kid, st = eng.vkey_add_rsa(bc.encode_key(m, ex))
        assert st == bc.OK, (i, st)
        assert class_words(m.bit_length()) == w
        keys.append((kid, m, ex))
    assert len(keys) == 8 and {k[2] for k in keys} == set(EXPONENTS)
    ow = 96 if w != 96 else 64  # a live key of another class
    other, st = eng.vkey_add_rsa(bc.encode_key(rng.getrandbits(32 * ow) | 1 | (1 << (32 * ow - 1)), 65537))
    gone, st2 = eng.vkey_add_rsa(bc.encode_key(mods[3], 3))
    assert st == bc.OK and st2 == bc.OK
    eng.vkey_remove(gone)
    try:
        for n in (1, 7, 9, 33, 200):
            ids, ins, want = [], [], []
            for i in range(n):
                kid, m, ex = keys[(i + n) % 8]
                a = [m - 1, 0, 1, rng.randrange(m)][(i // 8 + i) % 4]
                ids.append(kid)
                ins.append(a)
                want.append(pow(a, ex, m))
            got = run_public_op_keyed(eng, torch_dev, w, ids, ins)
            assert got == want, (w, n, [i for i in range(n) if got[i] != want[i]][:8])
        # contract violations and ids that name no key of this class: zero rows, neighbours exact
        r = 1 << (32 * w)
        ids, ins, want = [], [], []
        for i in range(40):
            kid, m, ex = keys[i % 8]
            a = rng.randrange(m)
            kind = i % 10
            if kind == 1:
                a, z = m, True
            elif kind == 3 and m + 2 < r:
                a, z = m + 2, True
            elif kind == 4 and m < r - 1:
                a, z = r - 1, True
            elif kind == 5:
                kid, z = [NO_ID, 0, (kid & 63) | ((kid >> 6) + 5) << 6][i // 10 % 3], True  # never issued
            elif kind == 6:
                kid, z = gone, True
            elif kind == 8:
                kid, z = other, True
            else:
                z = False
            ids.append(kid)
            ins.append(a)
            want.append(0 if z else pow(a, ex, m))
        got = run_public_op_keyed(eng, torch_dev, w, ids, ins)
        assert got == want, (w, [i for i in range(40) if got[i] != want[i]][:8])
        assert sum(x == 0 for x in want) >= 14 and sum(x != 0 for x in want) >= 14
    finally:
        for kid, _, _ in keys:
            eng.vkey_remove(kid)
        eng.vkey_remove(other)


# ---- 2. golden vectors ----------------------------------------------------------------------------
def test_declined_and_malformed_keys_take_no_slot(eng, golden, reg):
    keys, vs = golden
    status_of = {v["key"]: v["status"] for v in vs if v["cat"] in ("declined_key", "malformed_key")}
    # fill the count of live keys by what it is now: a failed add must not change it
    seen = 0
    for i, k in enumerate(keys):
        if i in reg:
            continue
        want = bc.decode_key(k["der"])
        assert isinstance(want, int) and want in (bc.BAD_KEY, bc.UNSUPPORTED)
        assert eng.vkey_add_rsa(k["der"]) == (NO_ID, want), k["name"]
        if i in status_of:
            assert status_of[i] == want  # the vector's status of a generic lane with that key
        seen += 1
    assert seen == 10
    assert eng.vkey_add_rsa(b"") == (NO_ID, bc.BAD_KEY)
    # no slot was taken: 64 - 11 more keys fit, the next one does not
    from corda_amd import _lib
    der = keys[0]["der"]
    extra = []
    for _ in range(_lib.VKEY_MAX_KEYS - len(reg)):
        kid, st = eng.vkey_add_rsa(der)
        assert st == bc.OK
        extra.append(kid)
    kid_c, kst = ctypes.c_uint32(), ctypes.c_uint8()
    assert _lib.lib().cordahip_vkey_add_rsa(eng.ctx, der, len(der), ctypes.byref(kid_c), ctypes.byref(kst)) == \
        _lib.ERR_OUT_OF_MEMORY
    for kid in extra:
        eng.vkey_remove(kid)
    # a NULL pointer is an argument error
    assert _lib.lib().cordahip_vkey_add_rsa(eng.ctx, None, 0, ctypes.byref(kid_c), ctypes.byref(kst)) == \
        _lib.ERR_INVALID_ARG
    assert _lib.lib().cordahip_vkey_add_rsa(eng.ctx, der, len(der), None, ctypes.byref(kst)) == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("is_valid", (False, True))
def test_golden_vectors_keyed_batch(eng, golden, reg, is_valid):
    """every vector of a registered key in one batch: the three classes interleaved"""
    keys, vs = golden
    lanes = [v for v in vs if v["key"] in reg]
    random.Random(18).shuffle(lanes)
    assert len(lanes) >= 170
    assert {class_words(keys[v["key"]]["n"].bit_length()) for v in lanes[:16]} == set(CLASSES)  # interleaved
    st, verdict = eng.rsa_verify_keyed_batch([reg[v["key"]] for v in lanes], [v["sig"] for v in lanes],
                                             [v["msg"] for v in lanes], is_valid=is_valid)
    name = "status_is_valid" if is_valid else "status"
    bad = [(i, v["cat"], keys[v["key"]]["name"], int(s), v[name]) for i, (v, s) in enumerate(zip(lanes, st))
           if int(s) != v[name]]
    assert not bad, bad[:20]
    assert verdict_bits(verdict, len(lanes)) == [int(v[name] == bc.OK) for v in lanes]
    assert sum(v["cat"] == "top_bit" and v[name] == bc.OK for v in lanes) >= 5  # the BC-lenient rule is exercised


# ---- 3. keyed equals generic -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus(golden, reg):
    """240 fresh CRT-signed lanes over the signing keys, every fifth signature bit-flipped, and the
    length edge cases; computed once"""
    keys, _ = golden
    ks = [(i, k) for i, k in enumerate(keys) if "d" in k and i in reg]
    assert len(ks) >= 10
    rng = random.Random(0xC0DB)
    lanes = []  # (key index, sig, msg)
    for i in range(240):
        ki, k = ks[i % len(ks)]
        m = rng.randbytes(1 + (i * 7) % 199)
        lanes.append((ki, fresh_signature(rng, k, m, flip=i % 5 == 4), m))
    for j, (ki, k) in enumerate(ks):
        m = rng.randbytes(20 + j)
        sig = fresh_signature(rng, k, m)
        kl = (k["n"].bit_length() + 7) // 8
        lanes += [(ki, sig[:kl - 1], m), (ki, b"\x00" + sig, m), (ki, b"", m), (ki, sig, b""), (ki, b"", b""),
                  (ki, sig + b"\x00" * 600, m)]
    assert {len(l[2]) for l in lanes[:240]} >= set(range(1, 200))
    return lanes


@pytest.mark.parametrize("is_valid", (False, True))
def test_keyed_equals_generic(eng, golden, reg, corpus, is_valid):
    keys, _ = golden
    ders = [keys[ki]["der"] for ki, _, _ in corpus]
    sigs = [s for _, s, _ in corpus]
    msgs = [m for _, _, m in corpus]
    want = [bc.verify(d, s, m, is_valid=is_valid) for d, s, m in zip(ders, sigs, msgs)]
    gen, gv = eng.verify_batch([RSA] * len(corpus), ders, sigs, msgs, is_valid=is_valid, rsa=True)
    st, verdict = eng.rsa_verify_keyed_batch([reg[ki] for ki, _, _ in corpus], sigs, msgs, is_valid=is_valid)
    assert [int(s) for s in st] == [int(s) for s in gen]
    assert [int(s) for s in st] == want
    assert verdict_bits(verdict, len(corpus)) == verdict_bits(gv, len(corpus)) == [int(x == bc.OK) for x in want]
    assert sum(x == bc.OK for x in want[:240]) == 240 - 48
    assert (bc.EMPTY in want) == (not is_valid) and bc.BAD_SIG in want


# ---- 3b. the host call's chunk and launch loops -----------------------------------------------------
GUARD = 64


def csr(items):
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(items) or b"\0", np.uint8).copy(), off


def run_keyed_arrays(e, ids, sb, so, mb, mo, is_valid=False, with_verdict=True):
    """cordahip_rsa_verify_keyed over a batch's arrays as they cross (ids uint32 [n], bytes with uint64
    [n + 1] offsets), status and verdict between 0xA5 guards. Returns (status, verdict words or None)."""
    from corda_amd import _lib
    n = len(ids)
    words = (n + 63) // 64
    st = np.full(GUARD + n + GUARD, 0xA5, np.uint8)
    vd = np.full(GUARD + words * 8 + GUARD, 0xA5, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    b = _lib.KeyedSigBatch(n, p(ids), p(sb), p(so), p(mb), p(mo), p(st) + GUARD, p(vd) + GUARD if with_verdict else None,
                           _lib.FLAG_IS_VALID if is_valid else 0, int(so[n]), int(mo[n]))
    assert _lib.lib().cordahip_rsa_verify_keyed(e.ctx, ctypes.byref(b)) == 0
    for buf in (st, vd):
        assert (buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all()
    if not with_verdict:  # a NULL verdict pointer: statuses only
        assert (vd == 0xA5).all()
        return st[GUARD:GUARD + n].copy(), None
    return st[GUARD:GUARD + n].copy(), vd[GUARD:GUARD + words * 8].copy().view(np.uint64)


def verdict_words(statuses):
    """the words a call owes for these statuses: bit i = lane i is OK, zero bits past n"""
    w = np.zeros((len(statuses) + 63) // 64, np.uint64)
    for i, x in enumerate(statuses):
        if int(x) == bc.OK:
            w[i // 64] |= np.uint64(1 << (i % 64))
    return w


@pytest.fixture(scope="module")
def three_chunks(eng, golden, reg, corpus):
    """130 lanes for CORDAHIP_HOST_CHUNK=64 (chunks of 64 / 64 / 2): the corpus' first lanes, their keys
    alternating between the width classes, with a signature longer than every slot, an empty message
    and the corpus' flipped signatures; ids nobody was issued on both sides of each chunk edge. The
    statuses wanted are the generic path's for the same lanes with the keys spelled out (asked once,
    under the default chunk size), UNKNOWN_KEY for the unknown ids."""
    keys, _ = golden
    lanes = [list(l) for l in corpus[:130]]
    lanes[10][1] = lanes[10][1] + b"\x00" * 600
    lanes[70][2] = b""
    unknown = (63, 64, 127, 128)
    for a in (0, 64):  # lanes of at least two classes alternate within each full chunk
        cls = [class_words(keys[l[0]]["n"].bit_length()) for l in lanes[a:a + 64]]
        assert len(set(cls)) >= 2 and sum(x != y for x, y in zip(cls, cls[1:])) >= 16
    assert sum(i % 5 == 4 for i in range(130)) >= 20  # the corrupted signatures
    ids = np.array([(reg[l[0]] & 63) | 0x3FFFF << 6 if i in unknown else reg[l[0]] for i, l in enumerate(lanes)],
                   np.uint32)
    sigs, msgs = [l[1] for l in lanes], [l[2] for l in lanes]
    want = {}
    for is_valid in (False, True):
        gen, _ = eng.verify_batch([RSA] * 130, [keys[l[0]]["der"] for l in lanes], sigs, msgs, is_valid=is_valid,
                                  rsa=True)
        w = [UNKNOWN if i in unknown else int(x) for i, x in enumerate(gen)]
        assert {bc.OK, bc.BAD_SIG, UNKNOWN} <= set(w) and w[10] == bc.BAD_SIG and w[129] != UNKNOWN
        assert w[70] == (bc.BAD_SIG if is_valid else bc.EMPTY)
        want[is_valid] = w
    return (ids,) + csr(sigs) + csr(msgs), want


@pytest.mark.parametrize("is_valid", (False, True))
@pytest.mark.parametrize("with_verdict", (True, False))
def test_three_chunks_classes_interleaved(eng, three_chunks, monkeypatch, with_verdict, is_valid):
    """The chunk loop over a full, a second and a partial chunk, each grouped by class again, with and
    without verdict words; with them, the last word is partial and has no bit set past lane 129."""
    arrays, want = three_chunks
    monkeypatch.setenv("CORDAHIP_HOST_CHUNK", "64")
    st, vd = run_keyed_arrays(eng, *arrays, is_valid=is_valid, with_verdict=with_verdict)
    bad = [(i, int(s), w) for i, (s, w) in enumerate(zip(st, want[is_valid])) if int(s) != w]
    assert not bad, bad[:10]
    if with_verdict:
        assert vd.tolist() == verdict_words(want[is_valid]).tolist() and int(vd[2]) >> 2 == 0


def test_two_launches_one_class(eng, golden, reg):
    """2^15 + 65 lanes of the 2048-bit class in one chunk: a full launch of the keyed stage's 2^15 rows
    and a second of 65 (a partial wave). The golden lanes of that class tiled; four signatures that
    verify get a bit flipped, two on each side of row 2^15, and are judged by the Python model; every
    other lane wants its golden status (the generic path agrees with those: test_keyed_equals_generic)."""
    keys, vs = golden
    base = [v for v in vs if v["key"] in reg and class_words(keys[v["key"]]["n"].bit_length()) == 64]
    nb, n = len(base), (1 << 15) + 65
    assert nb >= 32 and sum(v["status"] == bc.OK for v in base) >= 8
    reps = -(-n // nb)
    tile = lambda a: np.tile(np.asarray(a), reps)[:n]  # noqa: E731
    sig_len, msg_len = tile([len(v["sig"]) for v in base]), tile([len(v["msg"]) for v in base])
    so, mo = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    so[1:], mo[1:] = np.cumsum(sig_len), np.cumsum(msg_len)
    sb = np.tile(np.frombuffer(b"".join(v["sig"] for v in base), np.uint8), reps)[:int(so[n])].copy()
    mb = np.tile(np.frombuffer(b"".join(v["msg"] for v in base), np.uint8), reps)[:int(mo[n])].copy()
    ids = tile([reg[v["key"]] for v in base]).astype(np.uint32)
    want = tile([v["status"] for v in base]).astype(np.uint8)
    ok = np.nonzero(want == bc.OK)[0]
    edge = int(np.searchsorted(ok, 1 << 15))
    flipped = [int(ok[0]), int(ok[edge - 1]), int(ok[edge]), int(ok[-1])]
    assert flipped[1] < (1 << 15) <= flipped[2] and (1 << 15) - flipped[1] <= nb and flipped[3] >= n - nb
    for i in flipped:
        sb[int(so[i + 1]) - 1] ^= 1
        v = base[i % nb]
        want[i] = bc.verify(keys[v["key"]]["der"], bytes(sb[int(so[i]):int(so[i + 1])]), v["msg"])
        assert want[i] == bc.BAD_SIG
    st, vd = run_keyed_arrays(eng, ids, sb, so, mb, mo)
    bad = np.nonzero(st != want)[0]
    assert not len(bad), [(int(i), int(st[i]), int(want[i])) for i in bad[:10]]
    assert vd.tolist() == verdict_words(want).tolist()


# ---- 4. the device call ------------------------------------------------------------------------------
def run_verify_keyed_device(e, torch_dev, w, ids, sigs, sls, msgs, msg_len):
    torch, dev = torch_dev
    n = len(ids)
    sg = np.zeros((n, 4 * w), np.uint8)
    for i, s in enumerate(sigs):
        sg[i, :min(len(s), 4 * w)] = np.frombuffer(s[:4 * w], np.uint8)
    mg = np.zeros((n, msg_len), np.uint8)
    for i, m in enumerate(msgs):
        mg[i] = np.frombuffer(m, np.uint8)
    t = lambda a, ty: torch.from_numpy(a.view(ty).copy()).to(dev)  # noqa: E731
    tk, ts, tl, tg = t(np.array(ids, np.uint32), np.int32), t(sg, np.uint8), t(np.array(sls, np.uint16), np.int16), \
        t(mg, np.uint8)
    status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    verdict = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    e.rsa_verify_keyed_device(tk, ts, tl, tg, status, verdict, stream=s)
    s.synchronize()
    return [int(x) for x in status.cpu().numpy()], verdict.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("w", CLASSES)
def test_verify_keyed_device(eng, torch_dev, golden, reg, ed_vectors, ec_vectors, w):
    """n = 1 and n = 131 on a torch stream: sig_len 0, k - 1, k, slot + 1, a flipped top byte; an unknown,
    a removed, an Ed25519, an ECDSA id and an RSA id of another class are UNKNOWN_KEY; verdict words."""
    keys, _ = golden
    ks = [(i, k) for i, k in enumerate(keys) if i in reg and "d" in k and class_words(k["n"].bit_length()) == w]
    others = [reg[i] for i, k in enumerate(keys) if i in reg and class_words(k["n"].bit_length()) != w]
    assert ks and others
    (ed_id, _), (ec_id, _) = other_family_ids(eng, ed_vectors, ec_vectors)
    gone, st = eng.vkey_add_rsa(ks[0][1]["der"])
    assert st == bc.OK
    eng.vkey_remove(gone)
    rng = random.Random(0x4D + w)
    msg_len = 32
    try:
        for n in (1, 131):
            ids, sigs, sls, msgs, want = [], [], [], [], []
            for i in range(n):
                ki, k = ks[i % len(ks)]
                kl = (k["n"].bit_length() + 7) // 8
                m = rng.randbytes(msg_len)
                sig = fresh_signature(rng, k, m)
                kid, length, st = reg[ki], len(sig), bc.OK
                kind = i % 12 if n > 1 else 0
                if kind == 1:
                    length, st = 0, bc.EMPTY
                elif kind == 2:  # the signature cut to k - 1 bytes: another integer
                    sig, length = sig[:kl - 1], kl - 1
                    st = bc.verify(k["der"], sig, m)
                elif kind == 3:
                    length, st = 4 * w + 1, bc.BAD_SIG  # beyond the slot: nothing past it is read
                elif kind == 4:
                    sig = bytes([sig[0] ^ 0x01]) + sig[1:]
                    st = bc.verify(k["der"], sig, m)
                elif kind in (5, 6, 7, 8, 9):
                    kid = [(reg[ki] & 63) | 0x3FFFF << 6, gone, ed_id, ec_id, others[i % len(others)]][kind - 5]
                    st = UNKNOWN
                    if i % 24 >= 12:
                        length = 0  # UNKNOWN_KEY comes before EMPTY
                ids.append(kid)
                sigs.append(sig)
                sls.append(length)
                msgs.append(m)
                want.append(st)
            got, vd = run_verify_keyed_device(eng, torch_dev, w, ids, sigs, sls, msgs, msg_len)
            assert got == want, [(i, g, x) for i, (g, x) in enumerate(zip(got, want)) if g != x][:10]
            assert verdict_bits(vd, n) == [int(x == bc.OK) for x in want]
            if n > 1:
                assert {bc.OK, bc.BAD_SIG, bc.EMPTY, UNKNOWN} <= set(want)
        # msg_len == 0: every lane with a live key is EMPTY, the others stay UNKNOWN_KEY
        ids = [reg[ks[0][0]], gone, reg[ks[-1][0]], others[0]]
        sig = fresh_signature(rng, ks[0][1], b"x")
        got, vd = run_verify_keyed_device(eng, torch_dev, w, ids, [sig] * 4, [len(sig)] * 4, [b""] * 4, 0)
        assert got == [bc.EMPTY, UNKNOWN, bc.EMPTY, UNKNOWN] and not any(verdict_bits(vd, 4))
    finally:
        eng.vkey_remove(ed_id)
        eng.vkey_remove(ec_id)
    # a width the call does not have is an argument error
    from corda_amd import _lib
    assert _lib.lib().cordahip_rsa_verify_keyed_device(eng.ctx, 0, None, None, None, None, 32, 80, 0, None, None,
                                                        None) == _lib.ERR_INVALID_ARG
    assert _lib.lib().cordahip_rsa_public_op_keyed_device(eng.ctx, 0, None, None, 32, 0, None, None) == \
        _lib.ERR_INVALID_ARG


def test_device_calls_before_any_rsa_key(torch_dev, golden):
    """no RSA key was ever added on the device: no table, every lane UNKNOWN_KEY, every raw row zero"""
    from corda_amd.engine import Engine
    keys, vs = golden
    v = next(v for v in vs if v["cat"] == "valid" and keys[v["key"]]["n"].bit_length() == 2048)
    with Engine(1) as e:
        before = e.device_mem(0)[0]
        ids = [0, 64, 65, NO_ID, 1 << 6, 7, 63 | 9 << 6, 128, 4096]
        got, vd = run_verify_keyed_device(e, torch_dev, 64, ids, [v["sig"]] * 9, [len(v["sig"])] * 9,
                                          [v["msg"][:8].ljust(8, b"\0")] * 9, 8)
        assert got == [UNKNOWN] * 9 and not any(verdict_bits(vd, 9))
        assert run_public_op_keyed(e, torch_dev, 64, ids, [5] * 9) == [0] * 9
        st, _ = e.rsa_verify_keyed_batch(ids, [v["sig"]] * 9, [v["msg"]] * 9)
        assert [int(s) for s in st] == [UNKNOWN] * 9
        e.trim()
        assert e.device_mem(0)[0] == before  # and nothing of the table exists


# ---- 5. the registry ---------------------------------------------------------------------------------
def test_registry_across_three_families(golden, ed_vectors, ec_vectors):
    from corda_amd import _lib
    from corda_amd.engine import Engine
    keys, vs = golden
    k0, k1 = keys[0], keys[3]  # two 2048-bit keys
    v0 = next(v for v in vs if v["key"] == 0 and v["status"] == bc.OK)
    v1 = next(v for v in vs if v["key"] == 3 and v["status"] == bc.OK)
    with Engine(1) as e:
        run = lambda ids, v: [int(s) for s in e.rsa_verify_keyed_batch(ids, [v["sig"]] * len(ids),  # noqa: E731
                                                                       [v["msg"]] * len(ids))[0]]
        a, st = e.vkey_add_rsa(k0["der"])
        assert st == bc.OK
        assert run([a], v0) == [bc.OK]
        # removed: unknown; remove of a dead id is an argument error
        e.vkey_remove(a)
        assert run([a], v0) == [UNKNOWN]
        assert _lib.lib().cordahip_vkey_remove(e.ctx, a) == _lib.ERR_INVALID_ARG
        # the slot again, under a new id and another key: the old id stays unknown
        b, st = e.vkey_add_rsa(k1["der"])
        assert st == bc.OK and b != a and (b & 63) == (a & 63)
        assert run([a, b], v1) == [UNKNOWN, bc.OK]
        assert run([b], v0) == [bc.BAD_SIG]  # k0's signature under k1
        # the other families' ids name no RSA key, and an RSA id no key of theirs
        (ed_id, ed), (ec_id, ec) = other_family_ids(e, ed_vectors, ec_vectors)
        assert run([ed_id, ec_id, b], v1) == [UNKNOWN, UNKNOWN, bc.OK]
        st, _ = e.verify_keyed_batch([b, ed_id], [ed["sig"]] * 2, [ed["msg"]] * 2)
        assert [int(s) for s in st] == [UNKNOWN, bc.OK]
        st, _ = e.ecdsa_verify_keyed_batch([b, ec_id], [ec["sig"]] * 2, [ec["msg"]] * 2)
        assert [int(s) for s in st] == [UNKNOWN, bc.OK]
        # an Ed25519 key into a slot an RSA key held: the RSA id is unknown to both calls
        e.vkey_remove(b)
        ed_b, st = e.vkey_add_ed25519(ed["pub"])
        assert st == bc.OK and (ed_b & 63) == (b & 63)
        assert run([b, ed_b], v1) == [UNKNOWN, UNKNOWN]
        # the pool filled across the three families: the 65th add of any is refused, the context stays usable
        live = [ed_id, ec_id, ed_b]
        rsa_live = []
        while len(live) < _lib.VKEY_MAX_KEYS:
            i = len(live)
            if i % 3 == 0:
                kid, st = e.vkey_add_rsa((k0, k1)[i % 2]["der"])
                rsa_live.append((kid, i % 2))
            elif i % 3 == 1:
                kid, st = e.vkey_add_ed25519(ed["pub"])
            else:
                kid, st = e.vkey_add_ecdsa(ec["scheme"], ec["pub"])
            assert st == bc.OK
            live.append(kid)
        assert len(set(live)) == _lib.VKEY_MAX_KEYS and len(rsa_live) >= 20
        kid_c, kst = ctypes.c_uint32(), ctypes.c_uint8()
        der = k0["der"]
        assert _lib.lib().cordahip_vkey_add_rsa(e.ctx, der, len(der), ctypes.byref(kid_c), ctypes.byref(kst)) == \
            _lib.ERR_OUT_OF_MEMORY
        assert _lib.lib().cordahip_vkey_add_ed25519(e.ctx, ed["pub"], ctypes.byref(kid_c), ctypes.byref(kst)) == \
            _lib.ERR_OUT_OF_MEMORY
        assert run([k for k, _ in rsa_live], v1) == [bc.OK if which else bc.BAD_SIG for _, which in rsa_live]
        e.vkey_remove(live.pop())
        kid, st = e.vkey_add_rsa(k1["der"])  # the freed slot is there again
        assert st == bc.OK and run([kid], v1) == [bc.OK]


# ---- 6. tickets ----------------------------------------------------------------------------------------
def test_tickets_keyed_and_generic(eng, golden, reg):
    """two keyed tickets and one generic rsa=True ticket outstanding at once"""
    keys, vs = golden
    lanes = [v for v in vs if v["key"] in reg]
    a, b2 = lanes[:90], lanes[60:]
    ids = lambda xs: [reg[v["key"]] for v in xs]  # noqa: E731
    t1 = eng.rsa_verify_keyed_batch(ids(a), [v["sig"] for v in a], [v["msg"] for v in a], async_=True)
    t2 = eng.rsa_verify_keyed_batch(ids(b2), [v["sig"] for v in b2], [v["msg"] for v in b2], is_valid=True, async_=True)
    t3 = eng.verify_batch([RSA] * len(a), [keys[v["key"]]["der"] for v in a], [v["sig"] for v in a],
                          [v["msg"] for v in a], rsa=True, async_=True)
    st3, v3 = t3.wait()
    st2, v2 = t2.wait()
    st1, v1 = t1.wait()
    assert [int(s) for s in st1] == [v["status"] for v in a]
    assert [int(s) for s in st2] == [v["status_is_valid"] for v in b2]
    assert [int(s) for s in st3] == [v["status"] for v in a]
    assert verdict_bits(v1, len(a)) == verdict_bits(v3, len(a)) == [int(v["status"] == bc.OK) for v in a]
    assert verdict_bits(v2, len(b2)) == [int(v["status_is_valid"] == bc.OK) for v in b2]


# ---- 7. memory -------------------------------------------------------------------------------------------
def test_memory_accounting(golden, ed_vectors, ec_vectors):
    from corda_amd import _lib
    from corda_amd.engine import Engine
    keys, vs = golden
    lanes = [v for v in vs if v["key"] in (0, 1, 2)][:48]
    with Engine(1) as e:
        other_family_ids(e, ed_vectors, ec_vectors)  # only Ed25519 / ECDSA keys: no RSA table
        e.trim()
        base = e.device_mem(0)[0]
        ids = {}
        for i in (0, 1, 2):
            ids[i], st = e.vkey_add_rsa(keys[i]["der"])
            assert st == bc.OK
            assert e.device_mem(0)[0] - base == _lib.RSA_VKEY_TABLE_BYTES  # the first add allocates it, once
        e.trim()
        assert e.device_mem(0)[0] - base == _lib.RSA_VKEY_TABLE_BYTES  # and trim keeps it
        st, _ = e.rsa_verify_keyed_batch([ids[v["key"]] for v in lanes], [v["sig"] for v in lanes],
                                         [v["msg"] for v in lanes])
        assert [int(s) for s in st] == [v["status"] for v in lanes]
        assert e.device_mem(0)[0] - base > _lib.RSA_VKEY_TABLE_BYTES  # the stage and the workspace are accounted
        e.trim()
        assert e.device_mem(0)[0] - base == _lib.RSA_VKEY_TABLE_BYTES
        st, _ = e.rsa_verify_keyed_batch([ids[v["key"]] for v in lanes], [v["sig"] for v in lanes],
                                         [v["msg"] for v in lanes])
        assert [int(s) for s in st] == [v["status"] for v in lanes]  # the keys survived the trim
