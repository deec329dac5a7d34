"""Routing of registered-key ECDSA lanes to the keyed verifier on the GPU (K15:
cordahip_vkey_set_routing_ecdsa, cordahip_vkey_route_stats_ecdsa) through every call that
reaches ec_verify_enqueue: the dense device call, the host generic batch, the host signed-tx
batch and the stream call. Every status is compared with the C oracle (or the golden vectors),
not only with the unrouted call; cordahip_vkey_route_stats_ecdsa shows which engine ran, and its
deltas are asserted exactly against a Python statement of the rule after every call. Outputs are
prefilled with 0xA5 and sit between guard bytes. Every test uses a context of its own, so the
session engine never changes path."""
import collections
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bc_ecdsa as bc
import ec_vkey_model as model
from corda_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_SIG, MALFORMED_SIG, BAD_KEY, UNSUPPORTED, EMPTY = _lib.OK, 1, 2, 3, 4, _lib.EMPTY
UNKNOWN = _lib.VERIFY_UNKNOWN_KEY
ED, K1, R1, SPHINCS = 4, 2, 3, 5
PAD = 100
A5_WORD = 0xA5A5A5A5A5A5A5A5
# ecdsa_vkey.hpp: 64 tables of 320 KiB and the two base points', 64 records of 64 bytes, 96 bytes of scratch
EC_VKEY_BYTES = 66 * 320 * 1024 + 64 * 64 + 96
# ecdsa_route.hpp: a 64-byte header, 64 gathered records of 72 bytes, 4 bytes per lane for at least 2^16 lanes
EC_ROUTE_SCRATCH = 64 + 64 * 72 + 4 * (1 << 16)


# ---- the rule, stated in Python ---------------------------------------------------------------
def encodings(scheme, key):
    """Both SEC1 encodings of the point that the registered bytes decode to (oracle/bc_ecdsa.py)."""
    x, y = bc.decode_point(bc.CURVES[scheme], key)
    unc = b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big")
    return {unc, bc.compress(unc)}


def keyed_rule(registered):
    """registered: (scheme, key bytes) of the live ECDSA keys. Returns is_keyed(scheme, key bytes):
    the scheme is a live record's and the bytes are one of that record's point's two encodings."""
    enc = {(s, e) for s, k in registered for e in encodings(s, k)}
    return lambda scheme, key: (scheme, bytes(key)) in enc


def verdict_bits(words, n):
    return np.array([(int(words[i >> 6]) >> (i & 63)) & 1 for i in range(n)], np.uint8)


def stats_delta(eng, fn):
    before = eng.vkey_route_stats_ecdsa()
    out = fn()
    after = eng.vkey_route_stats_ecdsa()
    return out, (after[0] - before[0], after[1] - before[1])


def oracle_batch(oracle, lanes):
    """oracle_ecdsa_verify_batch (doVerify rules) over (scheme, key, sig, msg) lanes; a scheme that is
    no ECDSA scheme is UNSUPPORTED (Crypto.kt:474) and is kept from the oracle."""
    n = len(lanes)
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64)  # noqa: E731
    buf = lambda xs: np.frombuffer(b"".join(xs) or b"\0", np.uint8).copy()  # noqa: E731
    sc = np.asarray([x[0] if x[0] in (K1, R1) else K1 for x in lanes], np.uint8)
    pubs, sigs, msgs = [x[1] for x in lanes], [x[2] for x in lanes], [x[3] for x in lanes]
    kb, ko, sb, so, mb, mo = buf(pubs), off(pubs), buf(sigs), off(sigs), buf(msgs), off(msgs)
    want = np.zeros(n, np.uint8)
    oracle.oracle_ecdsa_verify_batch(n, sc.ctypes.data, kb.ctypes.data, ko.ctypes.data, sb.ctypes.data, so.ctypes.data,
                                     mb.ctypes.data, mo.ctypes.data, want.ctypes.data, 8)
    for i, x in enumerate(lanes):
        if x[0] not in (K1, R1):
            want[i] = UNSUPPORTED
    return want


def gpu_sign(eng, schemes, seeds, msgs):
    """cordahip_ecdsa_sign_device: (keys as 65-byte SEC1, DER signatures); d = SHA-256(seed) mod n, so
    lanes that share a seed and a scheme share a key. msgs: [n, L] uint8, L > 0."""
    import torch
    dev = torch.device("cuda:0")
    n = len(schemes)
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8)).to(dev)  # noqa: E731
    keys = torch.zeros((n, 65), dtype=torch.uint8, device=dev)
    sigs = torch.zeros((n, 72), dtype=torch.uint8, device=dev)
    kl, sl = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
    eng.ecdsa_sign_device(up(schemes), up(np.frombuffer(b"".join(seeds), np.uint8).reshape(n, 32)), up(msgs), keys, kl,
                          sigs, sl, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    k, s, l = keys.cpu().numpy(), sigs.cpu().numpy(), sl.cpu().numpy()
    assert (kl.cpu().numpy() == 65).all()
    return [k[i].tobytes() for i in range(n)], [s[i, :l[i]].tobytes() for i in range(n)]


def ec_dense_call(eng, lanes, msg_len, with_verdict=True):
    """cordahip_ecdsa_verify_device over (scheme, key, sig, msg) lanes whose messages have msg_len
    bytes, outputs 0xA5 between guards. Returns the statuses; checks the guards, and (with_verdict)
    bit = status OK and zero bits past n."""
    import torch
    dev = torch.device("cuda:0")
    n = len(lanes)
    words = (n + 63) // 64
    K, S = np.zeros((n, 65), np.uint8), np.zeros((n, 72), np.uint8)
    for i, (_, key, sig, msg) in enumerate(lanes):
        assert len(key) <= 65 and len(sig) <= 72 and len(msg) == msg_len
        K[i, :len(key)] = np.frombuffer(key, np.uint8)
        S[i, :len(sig)] = np.frombuffer(sig, np.uint8)
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.uint8)).to(dev)  # noqa: E731
    t_msg = up(np.frombuffer(b"".join(x[3] for x in lanes), np.uint8).reshape(n, msg_len)) if msg_len \
        else torch.empty((n, 0), dtype=torch.uint8, device=dev)
    t_st = torch.full((PAD + n + PAD,), 0xA5, dtype=torch.uint8, device=dev)
    t_vd = torch.full((2 + words + 2,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device=dev)
    eng.ecdsa_verify_device(up([x[0] for x in lanes]), up(K), up([len(x[1]) for x in lanes]), up(S),
                            up([len(x[2]) for x in lanes]), t_msg, t_st[PAD:PAD + n],
                            t_vd[2:2 + words] if with_verdict else None, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    st_all, vd_all = t_st.cpu().numpy(), t_vd.cpu().numpy().view(np.uint64)
    assert (st_all[:PAD] == 0xA5).all() and (st_all[PAD + n:] == 0xA5).all()
    assert (vd_all[:2] == A5_WORD).all() and (vd_all[2 + words:] == A5_WORD).all()
    got = st_all[PAD:PAD + n].copy()
    if with_verdict:
        bits = verdict_bits(vd_all[2:2 + words], words * 64)
        assert np.array_equal(bits[:n], (got == OK).astype(np.uint8)) and not bits[n:].any()
    else:
        assert (vd_all == A5_WORD).all()
    return got


def device_mem(eng):
    u = ctypes.c_uint64()
    assert _lib.lib().cordahip_device_mem(eng.ctx, 0, ctypes.byref(u), None, None) == 0
    return u.value


def run_self(func, env):
    """`func` of this module in a fresh process (the variables in env are read once per process)."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import conftest; import test_gpu_ec_vkey_route as t; t.%s()"
            % (ROOT, os.path.join(ROOT, "tests"), func))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


# ---- 1. golden vectors -------------------------------------------------------------------
def test_golden_vectors_routed(ec_vectors):
    """Every golden lane, none left out. The lanes a dense call can carry (a key of at most 65 bytes,
    a signature of at most 72) run through cordahip_ecdsa_verify_device per message length, routing
    off and then on, in every round of registered keys; the 47 with longer signatures run through
    cordahip_sig_verify with routing on (the host's DER decision reaches K13 as its pre byte)."""
    from corda_amd.engine import Engine
    assert len(ec_vectors) == 832
    dense = [v for v in ec_vectors if len(v["pub"]) <= 65 and len(v["sig"]) <= 72]
    long_sig = [v for v in ec_vectors if not (len(v["pub"]) <= 65 and len(v["sig"]) <= 72)]
    assert len(long_sig) == 47 and all(len(v["sig"]) > 72 and len(v["pub"]) in (33, 65) for v in long_sig)
    by_len = collections.defaultdict(list)
    for v in dense:
        by_len[len(v["msg"])].append(v)
    assert set(by_len) == {0, 32}
    keys = list(dict.fromkeys((v["scheme"], v["pub"]) for v in ec_vectors))
    assert len(keys) == 280
    decodable = [k for k in keys if bc.decode_point(bc.CURVES[k[0]], k[1]) is not None]
    keyed_cats, rounds, long_keyed = collections.Counter(), 0, 0
    with Engine(1) as eng:
        for g in range(0, len(decodable), _lib.VKEY_MAX_KEYS):
            group = decodable[g:g + _lib.VKEY_MAX_KEYS]
            ids = []
            for k in group:
                kid, st = eng.vkey_add_ecdsa(*k)
                assert st == OK
                ids.append(kid)
            is_keyed = keyed_rule(group)
            for ml, vs in sorted(by_len.items()):
                lanes = [(v["scheme"], v["pub"], v["sig"], v["msg"]) for v in vs]
                golden = np.array([v["status"] for v in vs], np.uint8)
                eng.vkey_set_routing_ecdsa(False)
                off, d = stats_delta(eng, lambda: ec_dense_call(eng, lanes, ml))
                assert d == (0, 0)  # routing off: counted nowhere
                eng.vkey_set_routing_ecdsa(True)
                on, d = stats_delta(eng, lambda: ec_dense_call(eng, lanes, ml))
                for name, got in (("off", off), ("on", on)):
                    wrong = [(name, v["cat"], v["note"], int(s), v["status"]) for v, s in zip(vs, got) if s != v["status"]]
                    assert not wrong, wrong[:10]
                assert np.array_equal(on, golden) and UNKNOWN not in on
                keyed = [v for v in vs if is_keyed(v["scheme"], v["pub"])]
                assert d == (len(keyed), len(vs) - len(keyed)), (g, ml, d)
                for v in keyed:
                    keyed_cats[v["cat"]] += 1
            # the signatures a 72-byte slot cannot carry: the host batch, routed
            (st, _), d = stats_delta(eng, lambda: eng.verify_batch([v["scheme"] for v in long_sig],
                                                                   [v["pub"] for v in long_sig],
                                                                   [v["sig"] for v in long_sig],
                                                                   [v["msg"] for v in long_sig]))
            assert [int(s) for s in st] == [v["status"] for v in long_sig]
            keyed = [v for v in long_sig if is_keyed(v["scheme"], v["pub"])]
            assert d == (len(keyed), len(long_sig) - len(keyed))
            for v in keyed:
                keyed_cats[v["cat"]] += 1
            long_keyed += len(keyed)
            eng.vkey_set_routing_ecdsa(False)
            for kid in ids:
                eng.vkey_remove(kid)
            rounds += 1
    assert len(decodable) == 186 and rounds == 3  # 94 keys are not points (key_bitflip and the key_* categories)
    total = collections.Counter(v["cat"] for v in ec_vectors)
    for cat in total:
        if cat in ("valid", "valid_compressed", "high_s", "sig_bitflip") or cat.startswith(("der_", "r_", "s_")):
            assert keyed_cats[cat] > 0, cat
    for cat in ("key_y_plus_p", "key_hybrid", "key_len"):
        assert total[cat] == 2 and keyed_cats[cat] == 0, cat
    assert long_keyed > 0  # the host's DER decision on a long signature reached K13 as its pre byte


# ---- 2. partition edges --------------------------------------------------------------------
EDGE_SIZES = (1, 63, 64, 65, 5 * 64 + 37)
EDGE_CALLS = (4 * 5 + 3) * 4


def edge_patterns(n):
    """name -> is-keyed per lane; a keyed count of exactly 255 / 256 / 257 needs n above it."""
    pats = {"all_k": [True] * n, "all_u": [False] * n, "alternating": [(i >> 1) % 2 == 0 for i in range(n)],
            "k_last": [i == n - 1 for i in range(n)]}
    for c in (255, 256, 257):
        if n > c:  # the unkeyed lanes spread over the batch, keyed everywhere else
            u = set(int(x) for x in np.linspace(0, n - 1, n - c).round())
            assert len(u) == n - c
            pats["keyed_%d" % c] = [i not in u for i in range(n)]
    return pats


def partition_edges(eng, oracle):
    """One registered key and one unregistered key per curve; the curves alternate lane by lane, so
    every wave holds both. Keyed lanes carry the registered key in both encodings; the others rotate
    through the unregistered key (both encodings) and the registered key's near misses: the
    wrong-parity compressed twin, 04 || X || p - Y, the registered P-256 bytes under scheme byte 2,
    and one lane of scheme byte 4. Fresh signatures with 1 in 7 corrupted; every pattern x size x
    verdict NULL / non-NULL x msg_len 32 / 0. Returns the number of dense calls made."""
    nmax = max(EDGE_SIZES)
    msgs = [hashlib.sha256(b"ec-route-edge-%d" % i).digest() for i in range(nmax)]
    seeds = {(s, w): hashlib.sha256(b"ec-route-%d-%s" % (s, w)).digest() for s in (K1, R1) for w in (b"R", b"U")}
    order = [(s, w) for s in (K1, R1) for w in (b"R", b"U")]
    keys, sigs = gpu_sign(eng, [s for s, _ in order for _ in range(nmax)], [seeds[o] for o in order for _ in range(nmax)],
                          np.frombuffer(b"".join(msgs * 4), np.uint8).reshape(4 * nmax, 32))
    pub = {o: keys[j * nmax] for j, o in enumerate(order)}
    sig = {o: sigs[j * nmax:(j + 1) * nmax] for j, o in enumerate(order)}
    for o in order:  # 1 in 7 corrupted: a bit of s
        for i in range(3, nmax, 7):
            s = bytearray(sig[o][i])
            s[-1 - i % 5] ^= 1 << (i % 8)
            sig[o][i] = bytes(s)
    reg = [(K1, pub[(K1, b"R")]), (R1, bc.compress(pub[(R1, b"R")]))]  # one of them registered in compressed form
    ids = []
    for k in reg:
        kid, st = eng.vkey_add_ecdsa(*k)
        assert st == OK
        ids.append(kid)
    is_keyed = keyed_rule(reg)

    def lane(i, keyed, first_unkeyed):
        s = (K1, R1)[i & 1]
        r65, u65 = pub[(s, b"R")], pub[(s, b"U")]
        comp = (i >> 1) & 1
        if keyed:
            return (s, bc.compress(r65) if comp else r65, sig[(s, b"R")][i], msgs[i])
        if first_unkeyed:
            return (4, r65, sig[(s, b"R")][i], msgs[i])  # class "other": the registered bytes, no ECDSA scheme
        v = (i >> 1) % 6
        p = bc.CURVES[s].p
        if v == 2:  # the compressed encoding with the wrong parity: the negated point
            return (s, bytes([bc.compress(r65)[0] ^ 1]) + r65[1:33], sig[(s, b"R")][i], msgs[i])
        if v == 3:  # 04 || X || p - Y
            return (s, r65[:33] + (p - int.from_bytes(r65[33:], "big")).to_bytes(32, "big"), sig[(s, b"R")][i], msgs[i])
        if v == 4:  # the registered P-256 bytes under scheme byte 2 (and the other way round)
            return (s, pub[(5 - s, b"R")], sig[(5 - s, b"R")][i], msgs[i])
        return (s, bc.compress(u65) if comp else u65, sig[(s, b"U")][i], msgs[i])

    eng.vkey_set_routing_ecdsa(True)
    calls, seen, variants = 0, set(), collections.Counter()
    for n in EDGE_SIZES:
        for name, flags in edge_patterns(n).items():
            first_u = flags.index(False) if False in flags else -1
            lanes32 = [lane(i, flags[i], i == first_u) for i in range(n)]
            for i, x in enumerate(lanes32):  # the pattern is the rule's answer
                assert is_keyed(x[0], x[1]) == flags[i], (n, name, i)
            for ml in (32, 0):
                lanes = [(s, k, g, m[:ml]) for s, k, g, m in lanes32]
                want = oracle_batch(oracle, lanes)
                if ml == 0:
                    assert set(want.tolist()) <= {EMPTY, BAD_KEY, UNSUPPORTED}
                elif n > 64 and name != "all_u":
                    assert (want == OK).any() and (want == BAD_SIG).any()
                for with_verdict in (True, False):
                    got, d = stats_delta(eng, lambda: ec_dense_call(eng, lanes, ml, with_verdict))
                    bad = np.nonzero(got != want)[0]
                    assert not len(bad), (n, name, ml, with_verdict, [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])
                    assert d == (sum(flags), n - sum(flags)), (n, name, ml, d)
                    calls += 1
            seen.add(name)
            variants.update(int(w) for w in oracle_batch(oracle, lanes32))
    assert seen == {"all_k", "all_u", "alternating", "k_last", "keyed_255", "keyed_256", "keyed_257"}
    assert {OK, BAD_SIG, BAD_KEY, UNSUPPORTED} <= set(variants)
    eng.vkey_set_routing_ecdsa(False)
    for kid in ids:
        eng.vkey_remove(kid)
    return calls


def test_partition_edges(oracle):
    from corda_amd.engine import Engine
    with Engine(1) as eng:
        assert partition_edges(eng, oracle) == EDGE_CALLS


def main_partition_edges():
    from conftest import load_oracle
    from corda_amd.engine import Engine
    with Engine(1) as eng:
        print(json.dumps({"calls": partition_edges(eng, load_oracle())}))


def test_partition_edges_small_workspace_subprocess():
    """A workspace of 128 slots: the generic list of the larger batches spans several chunks, and
    chunk sets fall wholly past the count (every lane keyed: all of them)."""
    assert run_self("main_partition_edges", {"CORDAHIP_ECDSA_WS_SLOTS": "128"})["calls"] == EDGE_CALLS


# ---- 3. the branches a table sum has and a ladder hardly ever reaches ----------------------------
FIXED_SCALARS = ["1", "n-1", "2^255-1", "2^255", "2^255+1", "0x80..", "0x81..", "0xff.."]
NEED = 8  # lanes per branch and curve, as in the K13 test


def mul_g(scheme, d):
    x, y = model.trace(scheme, None, d, 0)[0]
    return b"\x04" + x.to_bytes(32, "big") + y.to_bytes(32, "big")


def fixed_scalars(n):
    return [1, n - 1, (1 << 255) - 1, 1 << 255, (1 << 255) + 1, int.from_bytes(b"\x80" * 32, "big") % n,
            int.from_bytes(b"\x81" * 32, "big") % n, int.from_bytes(b"\xff" * 32, "big") % n]


def branch_lanes():
    """The construction of tests/test_gpu_ecdsa_verify_keyed.py's chosen-scalar lanes: a nonce with a
    zero top byte, keys d = 1 and n - 1, messages searched (modular arithmetic alone) until the sum of
    table entries meets an accumulator equal to the entry ("dbl"), equal to its inverse ("inf") and at
    infinity ("zero"); then chosen u1 and u2. (scheme, key, sig, msg, what) per lane."""
    lanes = []
    for scheme, c in bc.CURVES.items():
        n = c.n
        k = (int.from_bytes(hashlib.sha256(b"ec-vkey-nonce-%d" % scheme).digest(), "big") >> 8) % n
        r = bc._mul(c, k, c.G)[0] % n
        kinv = pow(k, -1, n)
        pub = {d: mul_g(scheme, d) for d in (1, n - 1)}
        qtab = {d: model.point_table(c, bc.decode_point(c, pub[d])) for d in (1, n - 1)}
        have = collections.Counter()
        i = 0
        while any(have[e] < NEED for e in ("dbl", "inf", "zero")):
            assert i < 60000, have
            d = (1, n - 1)[i & 1]
            msg = hashlib.sha256(b"ec-vkey-branch-%d-%d" % (scheme, i)).digest()
            i += 1
            e = int.from_bytes(hashlib.sha256(msg).digest(), "big") % n
            s = kinv * (e + r * d) % n
            if s == 0:
                continue
            w = pow(s, -1, n)
            _, ev = model.scalar_trace(n, d, e * w % n, r * w % n)
            hit = [x for x in ("dbl", "inf", "zero") if ev[x] and have[x] < NEED]
            if not hit:
                continue
            pt, pev = model.trace(scheme, qtab[d], e * w % n, r * w % n)  # the condition, through the point model
            assert pev == ev and pt is not None and pt[0] % n == r
            for x in ("dbl", "inf", "zero"):
                have[x] += bool(pev[x])
            lanes.append((scheme, pub[d], bc.der_encode(r, s), msg, "search " + "+".join(hit)))
        assert all(have[x] >= NEED for x in ("dbl", "inf", "zero")), have
        for name, u in zip(FIXED_SCALARS, fixed_scalars(n)):
            for which in (1, 2):
                msg = hashlib.sha256(b"ec-vkey-chosen-%d-%s-%d" % (scheme, name.encode(), which)).digest()
                e = int.from_bytes(hashlib.sha256(msg).digest(), "big") % n
                if which == 1:
                    u1 = u
                    s = e * pow(u1, -1, n) % n
                    u2 = r * pow(s, -1, n) % n
                else:
                    u2 = u
                    s = r * pow(u2, -1, n) % n
                    u1 = e * pow(s, -1, n) % n
                d = (k - u1) * pow(u2, -1, n) % n
                assert d and s and (u1, u2)[which - 1] == u
                lanes.append((scheme, mul_g(scheme, d), bc.der_encode(r, s), msg, "u%d = %s" % (which, name)))
    return lanes


def test_exceptional_branches_routed(oracle):
    from corda_amd.engine import Engine
    lanes = branch_lanes()
    want = oracle_batch(oracle, lanes)
    assert (want == OK).all(), [lanes[i][4] for i in np.nonzero(want != OK)[0]]
    keys = list(dict.fromkeys((x[0], x[1]) for x in lanes))
    assert len(keys) == 2 * (2 + 16) <= _lib.VKEY_MAX_KEYS
    n = len(lanes)
    with Engine(1) as eng:
        for i, k in enumerate(keys):  # every other key registered in compressed form: the lanes carry 65 bytes
            kid, st = eng.vkey_add_ecdsa(k[0], bc.compress(k[1]) if i & 1 else k[1])
            assert st == OK
        eng.vkey_set_routing_ecdsa(True)
        got, d = stats_delta(eng, lambda: ec_dense_call(eng, [x[:4] for x in lanes], 32))
        wrong = [(x[0], x[4], int(g)) for x, g in zip(lanes, got) if g != OK]
        assert not wrong, wrong[:10]
        assert d == (n, 0)
        # a flipped message on every lane must reject, through the same branches' neighbourhood
        flipped = [(x[0], x[1], x[2], bytes([x[3][0] ^ 1]) + x[3][1:]) for x in lanes]
        got, d = stats_delta(eng, lambda: ec_dense_call(eng, flipped, 32))
        assert (got == BAD_SIG).all() and np.array_equal(got, oracle_batch(oracle, flipped)) and d == (n, 0)


# ---- 4. the host generic batch ------------------------------------------------------------------
def csign(oracle, seed, msg):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_sign(seed, msg, len(msg), pub, sig)
    return pub.raw, sig.raw


def test_host_generic_batch_two_tickets(oracle):
    from corda_amd.engine import Engine
    with Engine(1) as eng:
        nec = 120
        msgs = [hashlib.sha512(b"ec-route-gen-%d" % i).digest()[:32] for i in range(nec)]
        who = [(K1, R1)[i & 1] for i in range(nec)]
        seed = {(s, w): hashlib.sha256(b"ec-route-gen-%d-%d" % (s, w)).digest() for s in (K1, R1) for w in (0, 1)}
        keys, sigs = gpu_sign(eng, who, [seed[(who[i], (i >> 1) & 1)] for i in range(nec)],
                              np.frombuffer(b"".join(msgs), np.uint8).reshape(nec, 32))
        reg = [(K1, keys[0]), (R1, keys[1])]  # lanes 0 and 1: the (scheme, 0) keys
        lanes = []
        for i in range(nec):
            k, g = keys[i], sigs[i]
            if i % 5 == 2:
                g = g[:-3] + bytes([g[-3] ^ 0x20]) + g[-2:]
            if i % 4 == 3:
                k = bc.compress(k)
            lanes.append((who[i], k, g, msgs[i]))
        seed_k, seed_u = hashlib.sha256(b"ec-route-gen-edK").digest(), hashlib.sha256(b"ec-route-gen-edU").digest()
        ed_k = csign(oracle, seed_k, b"x")[0]
        for i in range(60):  # Ed25519 lanes on a registered and an unregistered key
            m = hashlib.sha512(b"ec-route-gen-ed-%d" % i).digest()[:32 if i % 3 else 50]
            p, g = csign(oracle, seed_k if i % 2 else seed_u, m)
            if i % 5 == 1:
                g = g[:33] + bytes([g[33] ^ 0x20]) + g[34:]
            lanes.append((ED, p, g, m))
        long_der = bc.der_encode(1 << 600, 5)
        assert len(long_der) > 72
        lanes.append((K1, reg[0][1], long_der, msgs[0]))              # a DER signature above 72 bytes, registered key
        lanes.append((R1, reg[1][1], long_der + b"\0", msgs[1]))      # and one that is not DER
        lanes.append((K1, reg[0][1], b"", msgs[0]))                   # empty signature
        lanes.append((R1, bc.compress(reg[1][1]), sigs[1], b""))      # empty message
        lanes.append((K1, keys[2], sigs[2], b""))                     # the same on an unregistered key
        lanes.append((SPHINCS, reg[0][1], sigs[0], msgs[0]))          # an unsupported scheme
        lanes.append((K1, reg[0][1][:64], sigs[0], msgs[0]))          # a 64-byte key: decided on the host
        lanes.append((R1, reg[0][1], sigs[0], msgs[0]))               # secp256k1 bytes under the P-256 scheme byte
        order = np.random.default_rng(15).permutation(len(lanes))
        lanes = [lanes[i] for i in order]

        def want(is_valid):
            out = []
            for s, k, g, m in lanes:
                if s == ED:
                    f = oracle.oracle_ed25519_is_valid if is_valid else oracle.oracle_ed25519_verify
                    out.append(f(k, len(k), g, len(g), m, len(m)))
                elif s in (K1, R1):
                    f = oracle.oracle_ecdsa_is_valid if is_valid else oracle.oracle_ecdsa_verify
                    out.append(f(s, k, len(k), g, len(g), m, len(m)))
                else:
                    out.append(UNSUPPORTED)
            return np.array(out, np.uint8)

        w0, w1 = want(False), want(True)
        assert {OK, BAD_SIG, MALFORMED_SIG, BAD_KEY, UNSUPPORTED, EMPTY} <= set(w0.tolist())
        assert EMPTY not in set(w1.tolist()) and (w0 != w1).any()
        is_keyed = keyed_rule(reg)
        ec_dev = [x for x in lanes if x[0] in (K1, R1) and len(x[1]) in (33, 65)]  # the lanes the device sees
        ec_k = sum(is_keyed(x[0], x[1]) for x in ec_dev)
        ed_k_n = sum(x[0] == ED and x[1] == ed_k for x in lanes)
        ed_n = sum(x[0] == ED for x in lanes)
        assert 0 < ec_k < len(ec_dev) and 0 < ed_k_n < ed_n
        args = ([x[0] for x in lanes], [x[1] for x in lanes], [x[2] for x in lanes], [x[3] for x in lanes])
        off0, _ = eng.verify_batch(*args)
        assert np.array_equal(off0, w0), np.nonzero(off0 != w0)[0][:8]
        for k in reg:
            assert eng.vkey_add_ecdsa(*k)[1] == OK
        assert eng.vkey_add_ed25519(ed_k)[1] == OK
        eng.vkey_set_routing(True)
        eng.vkey_set_routing_ecdsa(True)
        ed_before = eng.vkey_route_stats()

        def two_tickets():
            t0 = eng.verify_batch(*args, async_=True)
            t1 = eng.verify_batch(*args, async_=True, is_valid=True)
            for t, w in ((t1, w1), (t0, w0)):
                st, vd = t.wait()
                bad = np.nonzero(st != w)[0]
                assert not len(bad), [(int(i), lanes[i][0], int(st[i]), int(w[i])) for i in bad[:8]]
                assert np.array_equal(verdict_bits(vd, len(lanes)), (w == OK).astype(np.uint8))
                assert UNKNOWN not in st

        _, d = stats_delta(eng, two_tickets)
        assert d == (2 * ec_k, 2 * (len(ec_dev) - ec_k))
        ed_after = eng.vkey_route_stats()
        assert (ed_after[0] - ed_before[0], ed_after[1] - ed_before[1]) == (2 * ed_k_n, 2 * (ed_n - ed_k_n))
        (st, _), d = stats_delta(eng, lambda: eng.verify_batch(*args))  # the synchronous call
        assert np.array_equal(st, w0) and d == (ec_k, len(ec_dev) - ec_k)


# ---- 5. the host signed-tx batch ----------------------------------------------------------------
NTX = 300
NO_SIG_TX = 123


def test_host_signed_tx_two_tickets(oracle, monkeypatch):
    """300 cash-issue-shaped transactions of two signatures each over their ids -- an ECDSA notary's
    (registered; P-256, and secp256k1 for every fifth transaction), then a fresh key's -- signatures of
    each kind corrupted at chosen positions, one transaction without signatures."""
    from corda_amd.corpus import cash_issue_items
    from corda_amd.engine import Engine
    monkeypatch.setenv("CORDAHIP_TX_SIG_CHUNK", "100")  # several pipeline chunks per call
    rng = np.random.default_rng(1615)
    blob, items, _ = cash_issue_items(rng.integers(0, 256, (NTX, 32), dtype=np.uint8),
                                      rng.integers(0, 256, (NTX, 32), dtype=np.uint8), bytes(range(32)),
                                      rng.integers(1, 10**9, NTX), rng.integers(-2**63, 2**63 - 1, NTX))
    host_it = items.reshape(-1).copy()
    host_it["data"] += np.uint64(blob.ctypes.data)
    hb, ho = _lib.kryo_encode_array(host_it)
    leaves = [[hb[int(ho[5 * t + j]):int(ho[5 * t + j + 1])].tobytes() for j in range(5)] for t in range(NTX)]
    with Engine(1) as eng:
        ids, _ = eng.tx_ids(leaves)
        out = ctypes.create_string_buffer(32)
        for t in (0, NO_SIG_TX, NTX - 1):  # the ids themselves against the oracle
            flat = np.frombuffer(b"".join(leaves[t]), np.uint8).copy()
            off = np.zeros(6, np.uint64)
            off[1:] = np.cumsum([len(x) for x in leaves[t]])
            assert oracle.oracle_tx_id(flat.ctypes.data, off.ctypes.data, 5, out) == 0 and out.raw == ids[t].tobytes()
        txs = [t for t in range(NTX) if t != NO_SIG_TX]
        sch, seeds, m = [], [], []
        for t in txs:
            notary = K1 if t % 5 == 0 else R1
            sch += [notary, (K1, R1)[t & 1]]
            seeds += [hashlib.sha256(b"ec-route-notary-%d" % notary).digest(),
                      hashlib.sha256(b"ec-route-fresh-%d" % t).digest()]
            m += [ids[t].tobytes()] * 2
        keys, sigs = gpu_sign(eng, sch, seeds, np.frombuffer(b"".join(m), np.uint8).reshape(len(m), 32))
        per_tx, flat = [[] for _ in range(NTX)], []
        for j, t in enumerate(x for t in txs for x in (t, t)):
            q, sg = j & 1, sigs[j]
            if (q == 0 and t % 13 == 4) or (q == 1 and t % 17 == 6) or t == 200:  # t = 200: both
                sg = sg[:-2] + bytes([sg[-2] ^ 4]) + sg[-1:]
            per_tx[t].append((sch[j], keys[j], sg))
            flat.append((sch[j], keys[j], sg, m[j]))
        want_sig = oracle_batch(oracle, flat)
        tso = np.zeros(NTX + 1, np.int64)
        tso[1:] = np.cumsum([len(p) for p in per_tx])
        want_fb, want_tx = [], []
        for t in range(NTX):
            st = want_sig[tso[t]:tso[t + 1]]
            bad = np.nonzero(st != OK)[0]
            want_fb.append(int(bad[0]) if len(bad) else -1)
            want_tx.append(_lib.TX_NO_SIGNATURES if not len(st) else int(st[bad[0]]) if len(bad) else 0)
        assert (want_sig == OK).sum() > 500 and (want_sig != OK).sum() >= 40 and want_fb[200] == 0 and 1 in want_fb
        reg = [(K1, keys[0]), (R1, bc.compress(keys[2]))]  # transactions 0 (secp256k1) and 1 (P-256)
        assert sch[0] == K1 and sch[2] == R1
        is_keyed = keyed_rule(reg)
        n_k = sum(is_keyed(x[0], x[1]) for x in flat)
        assert n_k == NTX - 1 and len(flat) == 2 * (NTX - 1)
        for k in reg:
            assert eng.vkey_add_ecdsa(*k)[1] == OK
        eng.vkey_set_routing_ecdsa(True)

        def two_tickets():
            tickets = [eng.signed_tx_verify(leaves, per_tx, async_=True) for _ in range(2)]
            for t in reversed(tickets):
                got_ids, tst, fb, sst = t.wait()
                skip = np.arange(NTX) != NO_SIG_TX
                assert np.array_equal(got_ids[skip], ids[skip])
                assert np.array_equal(sst, want_sig), np.nonzero(sst != want_sig)[0][:8]
                assert np.array_equal(fb, np.array(want_fb)) and np.array_equal(tst, np.array(want_tx, np.uint8))

        _, d = stats_delta(eng, two_tickets)
        assert d == (2 * n_k, 2 * (len(flat) - n_k))


# ---- 6. the stream call -------------------------------------------------------------------------
def test_stream_call_is_routed(oracle, monkeypatch):
    """cordahip_stream_verify reaches ec_verify_enqueue chunk by chunk (chunks of 64 lanes here), so its
    ECDSA section is routed too: statuses against the oracle, the split in the stats."""
    from corda_amd.engine import Engine
    monkeypatch.setenv("CORDAHIP_STREAM_CHUNK", "64")
    n = 333
    msgs = [hashlib.sha256(b"ec-route-stream-%d" % i).digest() for i in range(n)]
    with Engine(1) as eng:
        sch = [(K1, R1)[i & 1] for i in range(n)]
        seeds = [hashlib.sha256(b"ec-route-stream-%d-%d" % (sch[i], 0 if i % 4 else 1 + i)).digest() for i in range(n)]
        keys, sigs = gpu_sign(eng, sch, seeds, np.frombuffer(b"".join(msgs), np.uint8).reshape(n, 32))
        lanes = []
        for i in range(n):
            g = sigs[i]
            if i % 6 == 5:
                g = g[:-1] + bytes([g[-1] ^ 8])
            lanes.append((sch[i], bc.compress(keys[i]) if i % 3 == 0 else keys[i], g, msgs[i]))
        reg = [(K1, keys[2]), (R1, keys[1])]
        is_keyed = keyed_rule(reg)
        n_k = sum(is_keyed(x[0], x[1]) for x in lanes)
        assert n_k == n - (n + 3) // 4
        want = oracle_batch(oracle, lanes)
        assert (want == OK).any() and (want == BAD_SIG).any()
        K, S = np.zeros((n, 65), np.uint8), np.zeros((n, 72), np.uint8)
        for i, x in enumerate(lanes):
            K[i, :len(x[1])] = np.frombuffer(x[1], np.uint8)
            S[i, :len(x[2])] = np.frombuffer(x[2], np.uint8)
        kl, sl = np.array([len(x[1]) for x in lanes], np.uint8), np.array([len(x[2]) for x in lanes], np.uint8)
        M = np.frombuffer(b"".join(msgs), np.uint8).reshape(n, 32).copy()
        ed = (np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8), np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8))
        for k in reg:
            assert eng.vkey_add_ecdsa(*k)[1] == OK
        for on, split in ((False, (0, 0)), (True, (n_k, n - n_k))):
            eng.vkey_set_routing_ecdsa(on)
            got = np.full(PAD + n + PAD, 0xA5, np.uint8)
            _, d = stats_delta(eng, lambda: eng.stream_verify(ed, (np.array(sch, np.uint8), K, kl, S, sl, M,
                                                                    got[PAD:PAD + n])))
            assert (got[:PAD] == 0xA5).all() and (got[PAD + n:] == 0xA5).all()
            assert np.array_equal(got[PAD:PAD + n], want), (on, np.nonzero(got[PAD:PAD + n] != want)[0][:8])
            assert d == split, (on, d)


# ---- 7. registry changes ---------------------------------------------------------------------
def test_registry_changes_under_routing(oracle):
    from corda_amd.engine import Engine
    n = 200
    msgs = [hashlib.sha256(b"ec-route-reg-%d" % i).digest() for i in range(n)]
    with Engine(1) as eng:
        sch = [(K1, R1)[(i >> 1) & 1] for i in range(n)]
        seeds = [hashlib.sha256(b"ec-route-reg-%d-%d" % (sch[i], 1 if i % 3 else 0)).digest() for i in range(n)]
        keys, sigs = gpu_sign(eng, sch, seeds, np.frombuffer(b"".join(msgs), np.uint8).reshape(n, 32))
        lanes = []
        for i in range(n):
            g = sigs[i]
            if i % 7 == 1:
                g = g[:-1] + bytes([g[-1] ^ 1])
            lanes.append((sch[i], bc.compress(keys[i]) if i % 5 == 0 else keys[i], g, msgs[i]))
        key_k1 = next(keys[i] for i in range(n) if sch[i] == K1 and i % 3)
        key_r1 = next(keys[i] for i in range(n) if sch[i] == R1 and i % 3)
        other_k1 = next(keys[i] for i in range(n) if sch[i] == K1 and i % 3 == 0)
        n_k1 = sum(keyed_rule([(K1, key_k1)])(x[0], x[1]) for x in lanes)
        n_r1 = sum(keyed_rule([(R1, key_r1)])(x[0], x[1]) for x in lanes)
        want = oracle_batch(oracle, lanes)
        assert (want == OK).any() and (want == BAD_SIG).any() and 0 < n_k1 and 0 < n_r1 and n_k1 + n_r1 < n

        def run():
            got, d = stats_delta(eng, lambda: ec_dense_call(eng, lanes, 32))
            assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
            assert UNKNOWN not in got
            return d

        assert eng.vkey_route_stats_ecdsa() == (0, 0)
        eng.vkey_set_routing_ecdsa(True)
        assert run() == (0, 0)  # no key registered: today's path, nothing counted
        ed_pub = csign(oracle, hashlib.sha256(b"ec-route-reg-ed").digest(), b"x")[0]
        ed_id, st = eng.vkey_add_ed25519(ed_pub)  # an Ed25519 key alone is no reason to route ECDSA lanes
        assert st == OK
        assert run() == (0, 0)
        assert eng.vkey_route_stats() == (0, 0)  # and Ed25519 routing is another switch
        unrouted = device_mem(eng)  # the workspace of n lanes is there already
        a, st = eng.vkey_add_ecdsa(K1, key_k1)
        assert st == OK
        assert device_mem(eng) - unrouted == EC_VKEY_BYTES  # the ECDSA tables keep their size
        assert run() == (n_k1, n - n_k1)
        # what routing adds to the device's account: the two cumulative counters and slot 0's scratch
        assert n < 1 << 16 and device_mem(eng) - unrouted == EC_VKEY_BYTES + 16 + EC_ROUTE_SCRATCH
        # the scratch leaves the account with the workspace; the counters stay, routing works again
        held, tot = device_mem(eng), eng.vkey_route_stats_ecdsa()
        assert _lib.lib().cordahip_trim(eng.ctx) == 0
        assert held - device_mem(eng) > EC_ROUTE_SCRATCH and eng.vkey_route_stats_ecdsa() == tot
        assert run() == (n_k1, n - n_k1)
        eng.vkey_remove(a)
        assert run() == (0, 0)  # the last ECDSA key removed: the same statuses from the generic engine, nothing counted
        other, st = eng.vkey_add_ecdsa(K1, bc.compress(other_k1))  # takes the old slot
        assert st == OK and (other & 63) == (a & 63)
        assert run() == (sum(keyed_rule([(K1, other_k1)])(x[0], x[1]) for x in lanes),
                         n - sum(keyed_rule([(K1, other_k1)])(x[0], x[1]) for x in lanes))
        eng.vkey_remove(other)
        r, st = eng.vkey_add_ecdsa(R1, key_r1)  # one curve only, the other one
        assert st == OK
        assert run() == (n_r1, n - n_r1)
        b, st = eng.vkey_add_ecdsa(K1, key_k1)  # the same bytes again: a new id, live
        assert st == OK and b != a
        assert run() == (n_k1 + n_r1, n - n_k1 - n_r1)
        c, st = eng.vkey_add_ecdsa(K1, bc.compress(key_k1))  # the same point live twice: either serves
        assert st == OK
        assert run() == (n_k1 + n_r1, n - n_k1 - n_r1)
        eng.vkey_remove(b)
        assert run() == (n_k1 + n_r1, n - n_k1 - n_r1)
        eng.vkey_set_routing_ecdsa(False)
        assert run() == (0, 0)
        assert ctypes.c_int(_lib.lib().cordahip_vkey_route_stats_ecdsa(eng.ctx, 7, None, None)).value == \
            _lib.ERR_INVALID_ARG
        k, g = ctypes.c_uint64(), ctypes.c_uint64()
        assert _lib.lib().cordahip_vkey_route_stats_ecdsa(eng.ctx, 7, ctypes.byref(k), ctypes.byref(g)) == \
            _lib.ERR_INVALID_ARG
        assert eng.vkey_route_stats() == (0, 0)


# ---- 8. the lock order ---------------------------------------------------------------------------
def test_trim_keyed_and_routed_calls_together(oracle):
    """cordahip_trim (every buffer lock, vkey_stage.mu last), cordahip_ecdsa_verify_keyed (vkey_stage.mu
    around vkey_mu), a routed ECDSA dense call (ec_mu around vkey_mu) and a routed Ed25519 dense call
    (ed_mu around vkey_mu) from four threads: one lock order, so all four finish, with the right
    statuses throughout and the exact final counts."""
    import threading
    import torch
    from corda_amd.engine import Engine
    n = 130
    msgs = [hashlib.sha256(b"ec-route-locks-%d" % i).digest() for i in range(n)]
    errors = []
    with Engine(1) as eng:
        sch = [(K1, R1)[i & 1] for i in range(n)]
        seeds = [hashlib.sha256(b"ec-route-locks-%d-%d" % (sch[i], 0 if i % 3 else 1 + i)).digest() for i in range(n)]
        keys, sigs = gpu_sign(eng, sch, seeds, np.frombuffer(b"".join(msgs), np.uint8).reshape(n, 32))
        sigs = [s if i % 9 else s[:-1] + bytes([s[-1] ^ 2]) for i, s in enumerate(sigs)]
        lanes = [(sch[i], keys[i], sigs[i], msgs[i]) for i in range(n)]
        want = oracle_batch(oracle, lanes)
        reg = [(K1, keys[2]), (R1, keys[1])]
        ids = {}
        for k in reg:
            ids[k], st = eng.vkey_add_ecdsa(*k)
            assert st == OK
        is_keyed = keyed_rule(reg)
        k_lanes = [i for i in range(n) if is_keyed(sch[i], keys[i])]
        assert 0 < len(k_lanes) < n
        # the Ed25519 side: a registered key on every other lane
        seed_k = hashlib.sha256(b"ec-route-locks-edK").digest()
        ed_pairs = [csign(oracle, seed_k if i % 2 else hashlib.sha256(b"ec-route-locks-edU%d" % i).digest(), msgs[i])
                    for i in range(n)]
        ed_pub_k = csign(oracle, seed_k, b"x")[0]
        ed_keys = np.frombuffer(b"".join(p for p, _ in ed_pairs), np.uint8).reshape(n, 32).copy()
        ed_sigs = np.frombuffer(b"".join(s for _, s in ed_pairs), np.uint8).reshape(n, 64).copy()
        ed_sigs[::11, 40] ^= 4
        ed_msgs = np.frombuffer(b"".join(msgs), np.uint8).reshape(n, 32).copy()
        ed_want = np.zeros(n, np.uint8)
        oracle.oracle_ed25519_verify_batch(n, ed_keys.ctypes.data, ed_sigs.ctypes.data, ed_msgs.ctypes.data, 32,
                                           ed_want.ctypes.data, 8)
        ed_k = sum(p == ed_pub_k for p, _ in ed_pairs)
        assert eng.vkey_add_ed25519(ed_pub_k)[1] == OK
        eng.vkey_set_routing(True)
        eng.vkey_set_routing_ecdsa(True)
        dev = torch.device("cuda:0")

        def guard(fn):
            def run():
                try:
                    for _ in range(12):
                        fn()
                except Exception as e:  # noqa: BLE001
                    errors.append(repr(e))
            return run

        def trim():
            assert _lib.lib().cordahip_trim(eng.ctx) == 0

        def keyed():
            st, _ = eng.ecdsa_verify_keyed_batch([ids[(sch[i], keys[i])] for i in k_lanes], [sigs[i] for i in k_lanes],
                                                 [msgs[i] for i in k_lanes])
            assert np.array_equal(st, want[k_lanes])

        def routed_ec():
            assert np.array_equal(ec_dense_call(eng, lanes, 32), want)

        def routed_ed():
            st = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
            eng.ed25519_verify_device(torch.from_numpy(ed_keys).to(dev), torch.from_numpy(ed_sigs).to(dev),
                                      torch.from_numpy(ed_msgs).to(dev), st, None, stream=torch.cuda.current_stream())
            torch.cuda.synchronize()
            assert np.array_equal(st.cpu().numpy(), ed_want)

        threads = [threading.Thread(target=guard(f), daemon=True) for f in (trim, keyed, routed_ec, routed_ed)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(60)
        assert not any(t.is_alive() for t in threads), "a call did not return"
        assert not errors, errors[:3]
        assert eng.vkey_route_stats_ecdsa() == (12 * len(k_lanes), 12 * (n - len(k_lanes)))
        assert eng.vkey_route_stats() == (12 * ed_k, 12 * (n - ed_k))
