"""Routing of registered-key RSA rows to the keyed exponentiation on the GPU (K20:
cordahip_vkey_set_routing_rsa, cordahip_vkey_route_stats_rsa) through every call that reaches
rsa_verify_enqueue. Every routed result is compared with the unrouted call on the same inputs AND
with the Python model (tests/golden/bc_rsa_pss.py); cordahip_vkey_route_stats_rsa shows which
kernel ran, and its deltas must equal the counts the test computes from the rule.

The dense call cordahip_rsa_pss_verify_device has no flags argument (doVerify rules only), so
CORDAHIP_FLAG_IS_VALID is met through the generic host batch, whose RSA section passes it on. No
public call hands pre-statuses to the RSA enqueue; rows that the prep decides are met as
sig_len 0, sig_len beyond the modulus and an even modulus (tests/test_rsa_route_check.py replays
decided rows of every kind through the route pass on the host)."""
import ctypes
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bc_rsa_pss as bc
from corda_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RSA, ED, K1 = 1, 4, 2
CLASSES = (64, 96, 128)
NO_ID = 0xFFFFFFFF


def class_words(bits):
    return 64 if bits <= 2048 else 96 if bits <= 3072 else 128


def to_words(x, w):
    return np.frombuffer(x.to_bytes(4 * w, "little"), dtype="<u4").astype(np.uint32)


def verdict_bits(verdict, n):
    return [(int(verdict[i // 64]) >> (i % 64)) & 1 for i in range(n)]


def load_keys():
    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        g = json.load(f)
    keys = []
    for k in g["keys"]:
        k = dict(k, der=bytes.fromhex(k["der"]))
        for name in ("n", "e", "d", "p", "q"):
            if name in k:
                k[name] = int(k[name], 16)
        if "d" in k and not isinstance(bc.decode_key(k["der"]), int):
            keys.append(k)
    return keys


def sign(rng, k, msg, flip=False):
    em = bc.encode_em(msg, k["n"].bit_length(), rng.randbytes(32))
    s = bc.sign_crt(em, k["p"], k["q"], k["d"])
    sig = bytearray(s.to_bytes((k["n"].bit_length() + 7) // 8, "big"))
    if flip:
        sig[rng.randrange(1, len(sig))] ^= 1 << rng.randrange(8)
    return bytes(sig)


_POOL = {}


def pooled(k, j, flip=False):
    """(msg, sig): one of 6 CRT signatures per key, made once (signing in Python is the slow part of
    these tests); flip: a bit of it flipped, which bit following j"""
    key = (k["n"], j % 6)
    if key not in _POOL:
        rng = random.Random(hash(key) & 0xFFFFFF)
        m = rng.randbytes(32)
        _POOL[key] = (m, sign(rng, k, m))
    m, sig = _POOL[key]
    if flip:
        b = bytearray(sig)
        b[1 + (j * 7) % (len(b) - 1)] ^= 1 << (j % 8)
        sig = bytes(b)
    return m, sig


class Row:
    """one row of a dense call: the modulus and exponent it carries, its signature, length and message"""

    def __init__(self, n, e, sig, msg, sig_len=None):
        self.n, self.e, self.sig, self.msg = n, e, sig, msg
        self.sig_len = len(sig) if sig_len is None else sig_len

    def model(self, w):
        """the status by the Python model: the key as the row spells it"""
        if self.sig_len > 4 * w:  # beyond the slot: longer than any modulus of the class
            return bc.BAD_SIG if self.n % 2 and self.n.bit_length() >= 1024 else bc.UNSUPPORTED
        return bc.verify(bc.encode_key(self.n, self.e), self.sig[:self.sig_len], self.msg)


def run_dense(e, w, rows, msg_len=32, with_verdict=True):
    import torch
    dev = torch.device("cuda:0")
    n = len(rows)
    sg = np.zeros((n, 4 * w), np.uint8)
    mg = np.zeros((n, msg_len), np.uint8)
    for i, r in enumerate(rows):
        sg[i, :min(len(r.sig), 4 * w)] = np.frombuffer(r.sig[:4 * w], np.uint8)
        mg[i] = np.frombuffer(r.msg, np.uint8)
    t = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a).view(ty).copy()).to(dev)  # noqa: E731
    tm = t(np.stack([to_words(r.n, w) for r in rows]), np.int32)
    te = t(np.array([r.e for r in rows], np.uint32), np.int32)
    ts, tl, tg = t(sg, np.uint8), t(np.array([r.sig_len for r in rows], np.uint16), np.int16), t(mg, np.uint8)
    status = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    verdict = torch.full(((n + 63) // 64,), -1, dtype=torch.int64, device=dev) if with_verdict else None
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    e.rsa_pss_verify_device(tm, te, ts, tl, tg, status, verdict, stream=s)
    s.synchronize()
    st = [int(x) for x in status.cpu().numpy()]
    return st, (verdict_bits(verdict.cpu().numpy().view(np.uint64), n) if with_verdict else None)


def rule_keyed(rows, w, live):
    """the rule, from the test's own books: live = {(words, e, n)} of the live records"""
    return sum((w, r.e, r.n) in live for r in rows)


def routed_equals_unrouted(e, w, rows, live, with_verdict=True):
    """both legs of one dense batch, the model, and the stats deltas"""
    want = [r.model(w) for r in rows]
    e.vkey_set_routing_rsa(False)
    before = e.vkey_route_stats_rsa()
    off, off_v = run_dense(e, w, rows, with_verdict=with_verdict)
    assert e.vkey_route_stats_rsa() == before  # routing off: counted nowhere
    e.vkey_set_routing_rsa(True)
    on, on_v = run_dense(e, w, rows, with_verdict=with_verdict)
    after = e.vkey_route_stats_rsa()
    e.vkey_set_routing_rsa(False)
    bad = [(i, on[i], off[i], want[i]) for i in range(len(rows)) if not on[i] == off[i] == want[i]]
    assert not bad, (w, len(rows), bad[:10])
    if with_verdict:
        assert on_v == off_v == [int(x == bc.OK) for x in want]
    k = rule_keyed(rows, w, live)
    moved = (after[0] - before[0], after[1] - before[1])
    assert moved == ((k, len(rows) - k) if live else (0, 0)), (w, len(rows), moved, k)
    return want


@pytest.fixture(scope="module")
def keys():
    ks = load_keys()
    assert len(ks) >= 10 and {class_words(k["n"].bit_length()) for k in ks} == set(CLASSES)
    return ks


@pytest.fixture(scope="module")
def eng():
    """a context of this module's own: its registry and its counters"""
    from corda_amd.engine import Engine
    with Engine(1) as e:
        yield e


def by_class(keys, w):
    return [k for k in keys if class_words(k["n"].bit_length()) == w]


def unregistered_for(keys, w, reg_keys):
    """keys whose valid signatures stay generic in a class-w call: the class' other keys, and -- the
    fixture has one 4096-bit key -- narrower keys, whose moduli sit zero-padded in the wider row"""
    rest = [k for k in by_class(keys, w) if all(k["n"] != r["n"] for r in reg_keys)]
    return rest or by_class(keys, w - 32)[:2]


def mixed_rows(rng, w, n, reg_keys, other_keys):
    """valid and bit-flipped CRT signatures over registered and unregistered keys, interleaved"""
    rows = []
    for i in range(n):
        pool = reg_keys if i % 2 == 0 or not other_keys else other_keys
        k = pool[(i // 2) % len(pool)]
        m, sig = pooled(k, i + n, flip=i % 3 == 2)
        rows.append(Row(k["n"], k["e"], sig, m))
    return rows


# ---- 1. the dense call, per class ---------------------------------------------------------------
@pytest.mark.parametrize("w", CLASSES)
def test_dense_routed_equals_unrouted_and_model(eng, keys, w):
    rng = random.Random(0x20 + w)
    ks = by_class(keys, w)
    reg_keys = ks[:max(1, len(ks) // 2)]
    other_keys = unregistered_for(keys, w, reg_keys)
    ids = []
    try:
        # routing on with no RSA key ever added: stats do not move, results are equal
        if eng.vkey_route_stats_rsa() == (0, 0):
            routed_equals_unrouted(eng, w, mixed_rows(rng, w, 9, reg_keys, other_keys), set())
            assert eng.vkey_route_stats_rsa() == (0, 0)
        for k in reg_keys:
            kid, st = eng.vkey_add_rsa(k["der"])
            assert st == bc.OK
            ids.append(kid)
        live = {(w, k["e"], k["n"]) for k in reg_keys}
        for n in (1, 8, 9, 64, 65, 257):
            rows = mixed_rows(rng, w, n, reg_keys, other_keys)
            want = routed_equals_unrouted(eng, w, rows, live, with_verdict=n != 9)
            if n >= 64:
                assert {bc.OK, bc.BAD_SIG} <= set(want)
        # routing off with keys registered: stats do not move (asserted inside), results equal the model
        eng.vkey_set_routing_rsa(False)
        rows = mixed_rows(rng, w, 65, reg_keys, other_keys)
        before = eng.vkey_route_stats_rsa()
        assert run_dense(eng, w, rows)[0] == [r.model(w) for r in rows]
        assert eng.vkey_route_stats_rsa() == before
    finally:
        eng.vkey_set_routing_rsa(False)
        for kid in ids:
            eng.vkey_remove(kid)


@pytest.mark.parametrize("w", CLASSES)
def test_misroute_probes_and_decided_rows(eng, keys, w):
    """Rows a wrong match would answer OK and the model answers BAD_SIG; rows the prep decides keep
    their unrouted statuses; a cleared, a doubled and a short key."""
    rng = random.Random(0x21 + w)
    k = next(x for x in by_class(keys, w) if x["e"] == 65537)
    kid, st = eng.vkey_add_rsa(k["der"])
    assert st == bc.OK
    live = {(w, k["e"], k["n"])}
    ids = [kid]
    try:
        m = rng.randbytes(32)
        sig = sign(rng, k, m)
        kl = (k["n"].bit_length() + 7) // 8
        hi = k["n"] ^ (1 << (k["n"].bit_length() - 2))  # the registered modulus with one high bit flipped
        mid = k["n"] ^ (1 << (16 * w + 3))              # ... with one middle bit flipped
        rows = [
            Row(k["n"], k["e"], sig, m),                         # 0 keyed, OK
            Row(hi, k["e"], sig, m),                             # 1 a misroute would say OK
            Row(k["n"], 3, sig, m),                              # 2 the registered modulus under e = 3
            Row(mid, k["e"], sig, m),                            # 3
            Row(k["n"], k["e"], sig, m, sig_len=0),              # 4 EMPTY on a registered key
            Row(k["n"], k["e"], sig + b"\0", m, sig_len=kl + 1),  # 5 longer than the modulus
            Row(k["n"], k["e"], sig, m, sig_len=4 * w + 1),      # 6 beyond the slot
            Row(k["n"] ^ 1, k["e"], sig, m),                     # 7 an even modulus: UNSUPPORTED
            Row(k["n"], k["e"], sig[:kl - 1], m),                # 8 another integer
            Row(k["n"], k["e"], sig, m),                         # 9 keyed, OK again
        ]
        want = routed_equals_unrouted(eng, w, rows, live)
        assert want[:4] == [bc.OK, bc.BAD_SIG, bc.BAD_SIG, bc.BAD_SIG]
        assert want[4:8] == [bc.EMPTY, bc.BAD_SIG, bc.BAD_SIG, bc.UNSUPPORTED] and want[9] == bc.OK
        assert rule_keyed(rows, w, live) == 6  # decided rows count by match
        # the same key registered twice: keyed, either record serves
        kid2, st = eng.vkey_add_rsa(k["der"])
        assert st == bc.OK and kid2 != kid
        ids.append(kid2)
        routed_equals_unrouted(eng, w, rows, live)
        # one copy removed: still keyed; both removed: generic, and with no live RSA key the stats stand still
        eng.vkey_remove(ids.pop())
        routed_equals_unrouted(eng, w, rows, live)
        eng.vkey_remove(ids.pop())
        routed_equals_unrouted(eng, w, rows, set())
    finally:
        eng.vkey_set_routing_rsa(False)
        for x in ids:
            eng.vkey_remove(x)


def test_short_key_in_wider_call_is_generic(eng, keys):
    """A registered 2048-bit key in a 96-word call verifies OK and counts as generic (its class is 64)."""
    rng = random.Random(0x22)
    k = next(x for x in by_class(keys, 64) if x["n"].bit_length() == 2048)
    k96 = by_class(keys, 96)[0]
    ids = []
    try:
        for key in (k, k96):
            kid, st = eng.vkey_add_rsa(key["der"])
            assert st == bc.OK
            ids.append(kid)
        live = {(64, k["e"], k["n"]), (96, k96["e"], k96["n"])}
        rows = []
        for i in range(10):
            key = (k, k96)[i % 2]
            m = rng.randbytes(32)
            rows.append(Row(key["n"], key["e"], sign(rng, key, m), m))
        want = routed_equals_unrouted(eng, 96, rows, live)
        assert want == [bc.OK] * 10 and rule_keyed(rows, 96, live) == 5
    finally:
        eng.vkey_set_routing_rsa(False)
        for x in ids:
            eng.vkey_remove(x)


def test_add_and_remove_between_enqueues_on_one_stream(eng, keys):
    """Two routed enqueues on one stream with an add, then a remove, between them and no wait: the stats
    follow the registry, the statuses never change."""
    import torch
    rng = random.Random(0x23)
    w = 96
    k = by_class(keys, w)[0]
    rows = []
    for i in range(70):
        m = rng.randbytes(32)
        rows.append(Row(k["n"], k["e"], sign(rng, k, m, flip=i % 4 == 1), m))
    want = [r.model(w) for r in rows]
    dev = torch.device("cuda:0")
    sg = np.stack([np.frombuffer(r.sig.ljust(4 * w, b"\0"), np.uint8) for r in rows])
    t = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a).view(ty).copy()).to(dev)  # noqa: E731
    tm, te = t(np.stack([to_words(r.n, w) for r in rows]), np.int32), t(np.array([r.e for r in rows], np.uint32), np.int32)
    ts, tl = t(sg, np.uint8), t(np.array([r.sig_len for r in rows], np.uint16), np.int16)
    tg = t(np.stack([np.frombuffer(r.msg, np.uint8) for r in rows]), np.uint8)
    outs = [torch.full((70,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(3)]
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    base = eng.vkey_route_stats_rsa()
    other, st = eng.vkey_add_rsa(by_class(keys, 64)[0]["der"])  # a live RSA key, so that every leg is counted
    assert st == bc.OK
    eng.vkey_set_routing_rsa(True)
    try:
        eng.rsa_pss_verify_device(tm, te, ts, tl, tg, outs[0], None, stream=s)  # k not registered: generic
        kid, st = eng.vkey_add_rsa(k["der"])
        assert st == bc.OK
        eng.rsa_pss_verify_device(tm, te, ts, tl, tg, outs[1], None, stream=s)  # keyed
        eng.vkey_remove(kid)
        eng.rsa_pss_verify_device(tm, te, ts, tl, tg, outs[2], None, stream=s)  # generic again
        s.synchronize()
        for o in outs:
            assert [int(x) for x in o.cpu().numpy()] == want
        after = eng.vkey_route_stats_rsa()
        assert (after[0] - base[0], after[1] - base[1]) == (70, 140)
    finally:
        eng.vkey_set_routing_rsa(False)
        eng.vkey_remove(other)


def test_invalid_arguments_and_memory(eng, keys):
    k, g = ctypes.c_uint64(), ctypes.c_uint64()
    lib = _lib.lib()
    assert lib.cordahip_vkey_route_stats_rsa(eng.ctx, 7, ctypes.byref(k), ctypes.byref(g)) == _lib.ERR_INVALID_ARG
    assert lib.cordahip_vkey_route_stats_rsa(eng.ctx, 0, None, ctypes.byref(g)) == _lib.ERR_INVALID_ARG
    assert lib.cordahip_vkey_route_stats_rsa(eng.ctx, 0, ctypes.byref(k), None) == _lib.ERR_INVALID_ARG
    # the scratch is counted and goes with the workspace; the counters and the table stay
    rng = random.Random(0x24)
    key = by_class(keys, 64)[0]
    kid, st = eng.vkey_add_rsa(key["der"])
    assert st == bc.OK
    try:
        rows = []
        for i in range(64):
            m = rng.randbytes(32)
            rows.append(Row(key["n"], key["e"], sign(rng, key, m), m))
        eng.trim()
        idle = eng.device_mem(0)[0]
        eng.vkey_set_routing_rsa(False)
        assert run_dense(eng, 64, rows)[0] == [bc.OK] * 64
        unrouted = eng.device_mem(0)[0]
        eng.trim()
        assert eng.device_mem(0)[0] == idle
        eng.vkey_set_routing_rsa(True)
        tot = eng.vkey_route_stats_rsa()
        assert run_dense(eng, 64, rows)[0] == [bc.OK] * 64
        routed = eng.device_mem(0)[0]
        assert routed - unrouted in (64 + 12 * 64, 64 + 12 * 64 + 16)  # the scratch; the counters once
        eng.trim()
        assert eng.device_mem(0)[0] - idle in (0, 16)
        assert eng.vkey_route_stats_rsa() == (tot[0] + 64, tot[1])  # the counters survived the trim
    finally:
        eng.vkey_set_routing_rsa(False)
        eng.vkey_remove(kid)


# ---- 2. the launch loop under a small workspace ---------------------------------------------------
def launch_loop_results(e, ks):
    """130 rows per class, routing off and on; keyed rows on both sides of rows 64 and 128, the launch
    edges of a 64-row workspace. The statuses, the model's and the keyed count per class."""
    out = {}
    for w in CLASSES:
        rng = random.Random(0x25 + w)
        kc = by_class(ks, w)
        reg, other = kc[0], unregistered_for(ks, w, [kc[0]])[-1]
        kid, st = e.vkey_add_rsa(reg["der"])
        assert st == bc.OK
        rows = []
        for i in range(130):
            key = reg if (i % 3 != 1 or i in (63, 64, 127, 128)) else other
            m, sig = pooled(key, i, flip=i % 5 == 4)
            rows.append(Row(key["n"], key["e"], sig, m))
        rows[3].sig_len = 0
        e.vkey_set_routing_rsa(False)
        off, off_v = run_dense(e, w, rows)
        before = e.vkey_route_stats_rsa()
        e.vkey_set_routing_rsa(True)
        on, on_v = run_dense(e, w, rows)
        after = e.vkey_route_stats_rsa()
        e.vkey_set_routing_rsa(False)
        e.vkey_remove(kid)
        assert on == off and on_v == off_v
        keyed = sum(r.n == reg["n"] for r in rows)
        assert (after[0] - before[0], after[1] - before[1]) == (keyed, 130 - keyed)
        assert all(rows[i].n == reg["n"] for i in (63, 64, 127, 128))
        out[str(w)] = {"status": on, "model": [r.model(w) for r in rows], "keyed": keyed}
    return out


def main_launch_loop():
    from corda_amd.engine import Engine
    with Engine(1) as e:
        print(json.dumps(launch_loop_results(e, load_keys())))


def run_self(func, env):
    """`func` of this module in a fresh process (the variables in env are read once per process)."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]; import conftest; import test_gpu_rsa_route as t; t.%s()"
            % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), func))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_launch_loop_small_workspace_subprocess(eng, keys):
    """CORDAHIP_RSA_WS_ROWS=64 in a child process: 130 rows are 3 launches (64, 64, 2), each with its own
    route pass and fresh counts. Results equal the uncapped run of this process."""
    assert "CORDAHIP_RSA_WS_ROWS" not in os.environ
    capped = run_self("main_launch_loop", {"CORDAHIP_RSA_WS_ROWS": "64"})
    uncapped = launch_loop_results(eng, keys)
    assert capped == uncapped
    for w in CLASSES:
        c = capped[str(w)]
        assert c["status"] == c["model"] and c["keyed"] >= 80
        assert {bc.OK, bc.BAD_SIG, bc.EMPTY} <= set(c["status"])


# ---- 3. the generic host batch ----------------------------------------------------------------------
@pytest.mark.parametrize("is_valid", (False, True))
def test_generic_batch_mixed_families(eng, keys, ed_vectors, ec_vectors, is_valid):
    """About 200 lanes of the three families, the three RSA classes, RSA routing on: statuses equal the
    unrouted batch and the model; the RSA stats equal the RSA rows that reached the device; the Ed25519
    and ECDSA route stats are untouched."""
    rng = random.Random(0x26)
    # lanes with a signature and a message: their status is the same under both flags values
    full = lambda v: len(v["sig"]) > 0 and len(v["msg"]) > 0 and v["status"] != bc.EMPTY  # noqa: E731
    ed = [v for v in ed_vectors if len(v["pub"]) == 32 and full(v)][:40]
    ec = [v for v in ec_vectors if len(v["pub"]) in (33, 65) and len(v["sig"]) <= 72 and full(v)][:40]
    reg_keys = [by_class(keys, w)[0] for w in CLASSES]
    other = [by_class(keys, 64)[-1], by_class(keys, 96)[-1], by_class(keys, 96)[-2]]
    lanes = []  # (scheme, key, sig, msg, want or None)
    for v in ed:
        lanes.append((ED, v["pub"], v["sig"], v["msg"], v["status"]))
    for v in ec:
        lanes.append((v["scheme"], v["pub"], v["sig"], v["msg"], v["status"]))
    device_rows = keyed_rows = 0
    for i in range(120):
        k = (reg_keys if i % 2 == 0 else other)[i % 3]
        m, sig = pooled(k, i, flip=i % 4 == 3)
        if i % 17 == 5:
            sig = b""          # decided by the host: never reaches the device
        elif i % 17 == 6:
            sig = sig + b"\0"  # longer than the modulus: decided by the host too
        st = bc.verify(k["der"], sig, m, is_valid=is_valid)
        on_device = not (sig == b"" and not is_valid) and len(sig) <= (k["n"].bit_length() + 7) // 8
        device_rows += on_device
        keyed_rows += on_device and any(k["n"] == r["n"] for r in reg_keys)
        lanes.append((RSA, k["der"], sig, m, st))
    rng.shuffle(lanes)
    args = ([l[0] for l in lanes], [l[1] for l in lanes], [l[2] for l in lanes], [l[3] for l in lanes])
    ids = []
    try:
        for k in reg_keys:
            kid, st = eng.vkey_add_rsa(k["der"])
            assert st == bc.OK
            ids.append(kid)
        eng.vkey_set_routing_rsa(False)
        off, off_v = eng.verify_batch(*args, is_valid=is_valid, rsa=True)
        ed_before, ec_before, before = eng.vkey_route_stats(), eng.vkey_route_stats_ecdsa(), eng.vkey_route_stats_rsa()
        eng.vkey_set_routing_rsa(True)
        on, on_v = eng.verify_batch(*args, is_valid=is_valid, rsa=True)
        after = eng.vkey_route_stats_rsa()
        assert [int(x) for x in on] == [int(x) for x in off] == [l[4] for l in lanes]
        assert verdict_bits(on_v, len(lanes)) == verdict_bits(off_v, len(lanes))
        assert (after[0] - before[0], after[1] - before[1]) == (keyed_rows, device_rows - keyed_rows)
        assert keyed_rows >= 40 and device_rows - keyed_rows >= 40
        assert eng.vkey_route_stats() == ed_before and eng.vkey_route_stats_ecdsa() == ec_before
    finally:
        eng.vkey_set_routing_rsa(False)
        for kid in ids:
            eng.vkey_remove(kid)
