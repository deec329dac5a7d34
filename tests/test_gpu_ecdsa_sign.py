"""ECDSA batch signing with registered keys on the GPU (K17: cordahip_signer_add_ecdsa,
cordahip_ecdsa_sign, cordahip_ecdsa_sign_submit, cordahip_ecdsa_sign_keyed_device) against
RFC 6979's vectors (tests/golden/rfc6979_vectors.json), tests/golden/ecdsa_sign_vectors.json
and the model tests/ecdsa_sign_model.py, byte for byte; every signature is also judged by
cordahip_sig_verify, the C oracle and the keyed verifier (K13). Outputs are prefilled with
0xA5 and have guard bytes, so a lane the library does not write, or a write outside the
arrays, shows."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ecdsa_sign_model as M
from corda_amd import _lib
from corda_amd._lib import lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OK, EMPTY, BAD_KEY = _lib.OK, _lib.EMPTY, 3
UNKNOWN, SKIPPED, FAILED = _lib.SIGN_UNKNOWN_KEY, _lib.SIGN_SKIPPED, _lib.SIGN_FAILED
GUARD = 64
SLOT = 72
SIGNTAB_BYTES = (2 * 64 * 8 * 20 + 4096 * 32 + 8 + 20) * 4  # comb tables, records, the add kernel's scratch


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(HERE, "golden", "ecdsa_sign_vectors.json")))
    for k in g["keys"]:
        k["d_int"], k["pub_b"] = int(k["d"], 16), bytes.fromhex(k["pub"])
    for c in g["cases"]:
        c["msg_b"], c["sig_b"] = bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"])
    return g


@pytest.fixture(scope="module")
def keys(engine, golden):
    """The golden keys registered on the session engine: [(key_id, scheme, d, pub)]; pub is the model's [d]G."""
    out = []
    for k in golden["keys"]:
        kid, st, pub = engine.signer_add_ecdsa(k["scheme"], k["d_int"].to_bytes(32, "big"))
        assert st == OK and pub == k["pub_b"], k["d"]
        assert engine.signer_family(kid) == k["scheme"]
        out.append((kid, k["scheme"], k["d_int"], pub))
    assert len({k[0] for k in out}) == len(out)
    yield out
    for kid, _, _, _ in out:
        engine.signer_remove(kid)
        assert engine.signer_family(kid) is None


def device_sign(engine, ids, msgs, gate=None, device=0, stream=None, msg_len=None):
    """Dense rows through the device call, outputs inside guard rows of 0xA5.
    Returns (sigs[n, 72], sig_len[n], status[n]) as numpy and the device tensors."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ids)
    L = len(msgs[0]) if msg_len is None else msg_len
    stream = stream or torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        t_ids = torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32).copy()).to(dev)
        t_msg = torch.from_numpy(np.frombuffer(b"".join(msgs), np.uint8).reshape(n, L).copy()).to(dev)
        t_gate = None if gate is None else torch.from_numpy(np.asarray(gate, np.uint8).copy()).to(dev)
        b_sig = torch.full((n + 2, SLOT), 0xA5, dtype=torch.uint8, device=dev)
        b_len = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        b_st = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        t_sig, t_len, t_st = b_sig[1:n + 1], b_len[GUARD:GUARD + n], b_st[GUARD:GUARD + n]
        engine.ecdsa_sign_keyed_device(t_ids, t_msg, t_sig, t_len, t_st, gate=t_gate, device=device, stream=stream)
    stream.synchronize()
    for b, lo, hi in ((b_sig, 1, n + 1), (b_len, GUARD, GUARD + n), (b_st, GUARD, GUARD + n)):
        h = b.cpu().numpy()
        assert (h[:lo] == 0xA5).all() and (h[hi:] == 0xA5).all(), "guard bytes overwritten"
    return t_sig.cpu().numpy(), t_len.cpu().numpy(), t_st.cpu().numpy(), (t_ids, t_msg, t_sig, t_len)


def rows_equal(sig, ln, i, want):
    """Row i is `want` (bytes; None: a zero row of length 0), zero-padded to the slot."""
    want = want or b""
    return int(ln[i]) == len(want) and sig[i].tobytes() == want + bytes(SLOT - len(want))


class HostBatch:
    """cordahip_ecdsa_sign_batch arrays with guard bytes around sig, sig_len and status, everything 0xA5."""

    def __init__(self, ids, msgs, gate=None):
        self.n = n = len(msgs)
        self.ids = np.asarray(ids, np.uint32)
        self.off = np.zeros(n + 1, np.uint64)
        self.off[1:] = np.cumsum([len(m) for m in msgs])
        self.msg = np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy()
        self.gate = None if gate is None else np.asarray(gate, np.uint8)
        self.sig_buf = np.full(GUARD + n * SLOT + GUARD, 0xA5, np.uint8)
        self.len_buf = np.full(GUARD + n + GUARD, 0xA5, np.uint8)
        self.st_buf = np.full(GUARD + n + GUARD, 0xA5, np.uint8)

    def batch(self, off=None, msg_bytes=None):
        p = lambda a: a.ctypes.data  # noqa: E731
        return _lib.EcdsaSignBatch(self.n, p(self.ids), p(self.msg), p(self.off if off is None else off),
                                   p(self.gate) if self.gate is not None else None, p(self.sig_buf) + GUARD,
                                   p(self.len_buf) + GUARD, p(self.st_buf) + GUARD,
                                   int(self.off[self.n]) if msg_bytes is None else msg_bytes)

    @property
    def sig(self):
        return self.sig_buf[GUARD:GUARD + self.n * SLOT].reshape(self.n, SLOT)

    @property
    def len(self):
        return self.len_buf[GUARD:GUARD + self.n]

    @property
    def st(self):
        return self.st_buf[GUARD:GUARD + self.n]

    def untouched(self):
        return all((b == 0xA5).all() for b in (self.sig_buf, self.len_buf, self.st_buf))

    def guards_intact(self):
        return all((b[:GUARD] == 0xA5).all() and (b[-GUARD:] == 0xA5).all()
                   for b in (self.sig_buf, self.len_buf, self.st_buf))


# ---- 1. registry -------------------------------------------------------------------------------------
def test_registry(engine, oracle, keys):
    good, scheme, d, pub = keys[6]
    msg = hashlib.sha256(b"registry").digest()
    want = M.sign(M.CURVES[scheme], d, msg)
    # what is not a key is data: BAD_KEY, no id, no slot taken
    probe, st, _ = engine.signer_add_ecdsa(3, (12345).to_bytes(32, "big"))
    engine.signer_remove(probe)
    for c in (M.K1, M.R1):
        for bad in (0, c.n, 2**256 - 1):
            kid, st, p = engine.signer_add_ecdsa(c.scheme, bad.to_bytes(32, "big"))
            assert (kid, st, p) == (_lib.SIGNER_NO_ID, BAD_KEY, None), (c.name, bad)
    again, st, _ = engine.signer_add_ecdsa(3, (12345).to_bytes(32, "big"))
    assert st == OK and (again & 4095) == (probe & 4095) and again != probe  # the bad keys took no slot
    engine.signer_remove(again)
    kid = ctypes.c_uint32()
    stb, pb = ctypes.c_uint8(), ctypes.create_string_buffer(65)
    for scheme_bad in (0, 1, 4, 5):
        assert lib().cordahip_signer_add_ecdsa(engine.ctx, scheme_bad, bytes(31) + b"\1", ctypes.byref(kid),
                                               ctypes.byref(stb), pb) == _lib.ERR_INVALID_ARG
    # a removed id, and the slot's next key
    d2 = int.from_bytes(hashlib.sha256(b"registry-2").digest(), "big") % M.K1.n
    removed, st, _ = engine.signer_add_ecdsa(2, (777).to_bytes(32, "big"))
    engine.signer_remove(removed)
    assert lib().cordahip_signer_remove(engine.ctx, removed) == _lib.ERR_INVALID_ARG
    reused, st, pub2 = engine.signer_add_ecdsa(2, d2.to_bytes(32, "big"))
    assert reused != removed and (reused & 4095) == (removed & 4095) and pub2 == M.public_key(M.K1, d2)
    never = 4095 | (77 << 12)
    sig, ln, st, _ = device_sign(engine, [good, removed, reused, never], [msg] * 4)
    assert [int(s) for s in st] == [OK, UNKNOWN, OK, UNKNOWN]
    assert rows_equal(sig, ln, 0, want) and rows_equal(sig, ln, 1, None) and rows_equal(sig, ln, 3, None)
    assert rows_equal(sig, ln, 2, M.sign(M.K1, d2, msg))
    # the two families do not answer for each other's ids
    ed, _ = engine.signer_add_ed25519(hashlib.sha256(b"registry-ed").digest())
    assert engine.signer_family(ed) == "ed25519"
    esig, est = engine.sign_batch([good, ed], [msg, msg])
    assert [int(s) for s in est] == [UNKNOWN, OK] and not esig[0].any()
    rows, lens, cst = engine.ecdsa_sign_batch([ed, good], [msg, msg])
    assert [int(s) for s in cst] == [UNKNOWN, OK] and rows_equal(rows, lens, 0, None) and rows_equal(rows, lens, 1, want)
    # an Ed25519 key that takes an ECDSA key's slot, and the other way round
    engine.signer_remove(reused)
    ed2, _ = engine.signer_add_ed25519(hashlib.sha256(b"registry-ed2").digest())
    assert (ed2 & 4095) == (reused & 4095)
    rows, lens, cst = engine.ecdsa_sign_batch([ed2, reused], [msg, msg])
    assert [int(s) for s in cst] == [UNKNOWN, UNKNOWN] and not rows.any() and not lens.any()
    engine.signer_remove(ed2)
    ec3, st, _ = engine.signer_add_ecdsa(3, d2.to_bytes(32, "big"))
    assert (ec3 & 4095) == (ed2 & 4095)
    esig, est = engine.sign_batch([ec3, ed2], [msg, msg])
    assert [int(s) for s in est] == [UNKNOWN, UNKNOWN] and not esig.any()
    rows, lens, cst = engine.ecdsa_sign_batch([ec3], [msg])
    assert cst[0] == OK and rows_equal(rows, lens, 0, M.sign(M.R1, d2, msg))
    engine.signer_remove(ec3)
    engine.signer_remove(ed)


# ---- 2. the device call ------------------------------------------------------------------------------
def test_rfc6979_vectors_on_the_device(engine, keys):
    vs = json.load(open(os.path.join(HERE, "golden", "rfc6979_vectors.json")))["vectors"]
    added = {}
    try:
        for v in vs:
            if (v["scheme"], v["x"]) not in added:
                kid, st, pub = engine.signer_add_ecdsa(v["scheme"], bytes.fromhex(v["x"]))
                assert st == OK and pub == M.public_key(M.CURVES[v["scheme"]], int(v["x"], 16))
                added[(v["scheme"], v["x"])] = kid
        for v in vs:  # "sample", "test" and "Satoshi Nakamoto" differ in length: one call each
            msg = v["msg"].encode()
            sig, ln, st, _ = device_sign(engine, [added[(v["scheme"], v["x"])]], [msg])
            assert st[0] == OK and rows_equal(sig, ln, 0, M.der_sig(int(v["r"], 16), int(v["s"], 16))), v["msg"]
    finally:
        for kid in added.values():
            engine.signer_remove(kid)


def test_golden_cases_on_the_device(engine, golden, keys):
    cases = golden["cases"]
    for L in sorted({len(c["msg_b"]) for c in cases}):  # dense rows: one call per message length
        sel = [c for c in cases if len(c["msg_b"]) == L]
        sig, ln, st, _ = device_sign(engine, [keys[c["key"]][0] for c in sel], [c["msg_b"] for c in sel])
        assert not st.any(), L
        bad = [i for i, c in enumerate(sel) if not rows_equal(sig, ln, i, c["sig_b"])]
        assert not bad, (L, bad[:10])


@pytest.fixture(scope="module")
def mixed(engine, keys):
    """300 lanes (one full 256-thread block and a partial one): both curves and six keys lane by lane,
    gated lanes and unknown ids among them; the expected signatures from the model, once."""
    n = 300
    use = [keys[i] for i in (0, 5, 2, 7, 3, 9)]  # secp256k1 and P-256 alternate
    never = 4095 | (55 << 12)
    ids, gate, want, st, who = [], [], [], [], []
    msgs = [hashlib.sha256(b"ecdsa-mixed-%d" % i).digest() for i in range(n)]
    for i in range(n):
        kid, scheme, d, pub = use[i % len(use)]
        g = 3 if i % 11 == 4 else 0
        unk = i % 13 == 6
        ids.append(never if unk else kid)
        gate.append(g)
        s = SKIPPED if g else UNKNOWN if unk else OK
        st.append(s)
        want.append(M.sign(M.CURVES[scheme], d, msgs[i]) if s == OK else None)
        who.append((scheme, pub))
    assert any(g and ids[i] == never for i, g in enumerate(gate))  # gated and unknown: SKIPPED first
    sig, ln, got, dev = device_sign(engine, ids, msgs, gate)
    return dict(n=n, ids=ids, msgs=msgs, gate=gate, want=want, st=st, who=who, sig=sig, len=ln, got=got, dev=dev)


def test_mixed_lanes_statuses_and_bytes(engine, oracle, mixed):
    m = mixed
    assert [int(s) for s in m["got"]] == m["st"]
    bad = [i for i in range(m["n"]) if not rows_equal(m["sig"], m["len"], i, m["want"][i])]
    assert not bad, bad[:10]
    ok = [i for i in range(m["n"]) if m["st"][i] == OK]
    assert len(ok) > 200 and {m["who"][i][0] for i in ok} == {2, 3}
    sigs = [m["sig"][i][:int(m["len"][i])].tobytes() for i in ok]
    # judged by the generic verifier (K2) ...
    vst, _ = engine.verify_batch([m["who"][i][0] for i in ok], [m["who"][i][1] for i in ok], sigs,
                                 [m["msgs"][i] for i in ok])
    assert not vst.any()
    # ... and by the C oracle
    for j, i in enumerate(ok):
        scheme, pub = m["who"][i]
        assert oracle.oracle_ecdsa_verify(scheme, pub, 65, sigs[j], len(sigs[j]), m["msgs"][i], 32) == 0, i
    # msg_len = 0: every ungated lane with a live key is EMPTY; the precedence holds
    zsig, zlen, zst, _ = device_sign(engine, m["ids"], [b""] * m["n"], m["gate"], msg_len=0)
    assert [int(s) for s in zst] == [EMPTY if s == OK else s for s in m["st"]]
    assert not zsig.any() and not zlen.any()
    # no gate at all
    sig, ln, st, _ = device_sign(engine, m["ids"][:70], m["msgs"][:70])
    assert [int(s) for s in st] == [UNKNOWN if i % 13 == 6 else OK for i in range(70)]


def test_keyed_verifier_accepts_the_signatures(engine, mixed):
    """K13 over the signatures of the mixed call, the same public keys registered as verification keys."""
    m = mixed
    vk = {}
    try:
        for scheme, pub in sorted(set(m["who"])):
            vid, st = engine.vkey_add_ecdsa(scheme, pub)
            assert st == OK
            vk[(scheme, pub)] = vid
        ok = [i for i in range(m["n"]) if m["st"][i] == OK]
        st, _ = engine.ecdsa_verify_keyed_batch([vk[m["who"][i]] for i in ok],
                                                [m["sig"][i][:int(m["len"][i])].tobytes() for i in ok],
                                                [m["msgs"][i] for i in ok])
        assert not st.any()
        # and a signature under the wrong key is refused
        st, _ = engine.ecdsa_verify_keyed_batch([vk[m["who"][ok[2]]]], [m["sig"][ok[0]][:int(m["len"][ok[0]])].tobytes()],
                                                [m["msgs"][ok[0]]])
        assert st[0] != OK
    finally:
        for vid in vk.values():
            engine.vkey_remove(vid)


# ---- 3. the host calls -------------------------------------------------------------------------------
def test_host_calls_over_the_golden_cases(engine, golden, keys):
    cases = golden["cases"]
    ids = [keys[c["key"]][0] for c in cases]
    msgs = [c["msg_b"] for c in cases]
    hb = HostBatch(ids, msgs)
    assert lib().cordahip_ecdsa_sign(engine.ctx, ctypes.byref(hb.batch())) == 0
    assert not hb.st.any() and hb.guards_intact()
    bad = [i for i, c in enumerate(cases) if not rows_equal(hb.sig, hb.len, i, c["sig_b"])]
    assert not bad, bad[:10]
    sig, ln, st = engine.ecdsa_sign_batch(ids, msgs, async_=True).wait()
    assert not st.any() and np.array_equal(sig, hb.sig) and np.array_equal(ln, hb.len)
    # gate bytes, an empty message and an unknown id through the host call
    gate = [int(i % 7 == 2) for i in range(len(cases))]
    msgs2 = [b"" if i % 10 == 5 else m for i, m in enumerate(msgs)]
    ids2 = [4095 | (9 << 12) if i % 17 == 3 else k for i, k in enumerate(ids)]
    hb2 = HostBatch(ids2, msgs2, gate)
    assert lib().cordahip_ecdsa_sign(engine.ctx, ctypes.byref(hb2.batch())) == 0
    for i, c in enumerate(cases):
        s = SKIPPED if gate[i] else UNKNOWN if i % 17 == 3 else EMPTY if i % 10 == 5 else OK
        assert hb2.st[i] == s and rows_equal(hb2.sig, hb2.len, i, c["sig_b"] if s == OK else None), i
    assert hb2.guards_intact()
    assert engine.ecdsa_sign_batch([], []) [2].size == 0


@pytest.mark.parametrize("submit", [False, True])
def test_bad_msg_off_is_invalid_arg(engine, golden, keys, submit):
    kid, scheme, d, _ = keys[8]
    msgs = [hashlib.sha256(b"bad-off-%d" % i).digest()[:8 + i] for i in range(12)]
    hb = HostBatch([kid] * 12, msgs)

    def run(batch):
        if not submit:
            return lib().cordahip_ecdsa_sign(engine.ctx, ctypes.byref(batch))
        t = ctypes.c_uint64()
        rc = lib().cordahip_ecdsa_sign_submit(engine.ctx, ctypes.byref(batch), ctypes.byref(t))
        return rc if rc != 0 else lib().cordahip_wait(engine.ctx, t.value, -1)

    dec = hb.off.copy()
    dec[5] = dec[6] + 3  # decreasing
    past = hb.off.copy()
    past[12] += 1        # one byte past the message buffer
    for bad in (hb.batch(off=dec), hb.batch(off=past), hb.batch(msg_bytes=int(hb.off[12]) - 1)):
        assert run(bad) == _lib.ERR_INVALID_ARG
        assert hb.untouched()  # nothing was written
    assert run(hb.batch()) == 0  # the context stays usable
    assert not hb.st.any() and hb.guards_intact()
    for i in (0, 5, 11):
        assert rows_equal(hb.sig, hb.len, i, M.sign(M.CURVES[scheme], d, msgs[i])), i


def test_small_chunks_two_tickets_in_a_subprocess():
    """CORDAHIP_HOST_CHUNK=256 in a fresh process: 700 lanes of mixed lengths run as three chunks, two
    tickets outstanding; tests/ecdsa_sign_worker.py compares every row with the device call's and a sample
    with the model."""
    env = dict(os.environ, CORDAHIP_HOST_CHUNK="256")
    p = subprocess.run([sys.executable, os.path.join(HERE, "ecdsa_sign_worker.py")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r == {"ok": True, "lanes": 700, "tickets": 2, "chunk": "256", "compared_with_device": 1400,
                 "compared_with_model": r["compared_with_model"]} and r["compared_with_model"] >= 28


# ---- 4. chains ---------------------------------------------------------------------------------------
def _pmt_ok_cases():
    cases = json.load(open(os.path.join(HERE, "golden", "pmt_vectors.json")))["cases"]
    out = {}
    for c in cases:
        if c["status"] == 0:
            out.setdefault(c["root"], ([bytes.fromhex(x) for x in c["leaves"]],
                                       [(t, bytes.fromhex(h) if h else None) for t, h in c["tokens"]],
                                       bytes.fromhex(c["root"])))
    return list(out.values())


def test_gate_from_filtered_tx_verify(engine, oracle, keys):
    """Verify the tear-offs, then sign only what verified: the statuses cordahip_filtered_tx_verify wrote gate
    the ECDSA device signer on one stream; resolve.verify_and_sign_filtered_transactions does the same."""
    import torch
    from corda_amd import resolve as R
    ftxs = _pmt_ok_cases()[:12]
    victim = 5
    leaves, toks, root = ftxs[victim]
    ftxs[victim] = (leaves, toks, bytes([root[0] ^ 1]) + root[1:])  # a root the tree does not hash to
    kid, scheme, d, pub = keys[1]
    status = engine.filtered_tx_verify(ftxs)
    assert [int(s) != 0 for s in status] == [t == victim for t in range(len(ftxs))]
    stream = torch.cuda.Stream()
    sig, ln, st, _ = device_sign(engine, [kid] * len(ftxs), [f[2] for f in ftxs], gate=status, stream=stream)
    for t, f in enumerate(ftxs):
        if t == victim:
            assert st[t] == SKIPPED and rows_equal(sig, ln, t, None)
        else:
            der = sig[t][:int(ln[t])].tobytes()
            assert st[t] == OK and der == M.sign(M.CURVES[scheme], d, f[2])
            assert oracle.oracle_ecdsa_verify(scheme, pub, 65, der, len(der), f[2], 32) == 0
    tx_status, sigs = R.verify_and_sign_filtered_transactions(engine, ftxs, kid)
    assert tx_status == [int(s) for s in status]
    assert sigs == [None if t == victim else sig[t][:int(ln[t])].tobytes() for t in range(len(ftxs))]
    with pytest.raises(R.NoSuchElementException):
        R.verify_and_sign_filtered_transactions(engine, ftxs, 4095 | (99 << 12))


def test_device_chain_commit_then_sign(engine, oracle, keys):
    """commit -> sign on one stream with no host round trip: the tx_status cordahip_commit_inputs_device
    writes is the ECDSA signer's gate."""
    import torch
    import commit_log_worker as W
    dev = torch.device("cuda:0")
    kid, scheme, d, pub = keys[7]
    lid = engine.commit_log_create(10)
    try:
        now, tol = 10**18, 10**9
        txs = [(W.h("etx", 0), 7, [W.ref(0), W.ref(1)], None),
               (W.h("etx", 1), 8, [W.ref(1)], None),                    # conflict with the one before it
               (W.h("etx", 2), 8, [W.ref(2)], (None, now - tol - 1)),   # out of window
               (W.h("etx", 3), 8, [W.ref(3)], None)]
        n = len(txs)
        flat = [r for tx in txs for r in tx[2]]
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(tx[2]) for tx in txs])
        absent = _lib.TW_SIDE_ABSENT
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_txid = to(np.frombuffer(b"".join(tx[0] for tx in txs), np.uint8).reshape(n, 32).copy())
        d_caller = to(np.array([tx[1] for tx in txs], np.int32))
        d_refs = to(engine._state_refs(flat).view(np.uint8).reshape(-1, 36)[:len(flat)].copy())
        d_from = to(np.array([absent if not tx[3] or tx[3][0] is None else tx[3][0] for tx in txs], np.int64))
        d_until = to(np.array([absent if not tx[3] or tx[3][1] is None else tx[3][1] for tx in txs], np.int64))
        d_st = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        d_cm = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        d_rs = torch.full((len(flat),), 0xA5, dtype=torch.uint8, device=dev)
        d_rb = torch.full((len(flat), 40), 0xA5, dtype=torch.uint8, device=dev)
        d_kid = to(np.full(n, kid, np.int64).astype(np.uint32).view(np.int32))
        d_sig = torch.full((n, SLOT), 0xA5, dtype=torch.uint8, device=dev)
        d_len = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        d_sst = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            engine.commit_inputs_device(lid, d_txid, d_caller, d_refs, to(off), d_st, d_cm, d_rs, d_rb, tw_from=d_from,
                                        tw_until=d_until, now_ns=now, tolerance_ns=tol, stream=stream)
            engine.ecdsa_sign_keyed_device(d_kid, d_txid, d_sig, d_len, d_sst, gate=d_st, stream=stream)
        stream.synchronize()
        assert [int(x) for x in d_st.cpu().numpy()] == [OK, _lib.COMMIT_CONFLICT, _lib.COMMIT_TIME_WINDOW_INVALID, OK]
        sig, ln, sst = d_sig.cpu().numpy(), d_len.cpu().numpy(), d_sst.cpu().numpy()
        assert [int(x) for x in sst] == [OK, SKIPPED, SKIPPED, OK]
        for t, tx in enumerate(txs):
            assert rows_equal(sig, ln, t, M.sign(M.CURVES[scheme], d, tx[0]) if sst[t] == OK else None), t
    finally:
        engine.commit_log_destroy(lid)


def test_notarise_with_a_p256_signer(engine, oracle, keys):
    """resolve.notarise_filtered_transactions with a P-256 signer id over 40 transactions with conflicts, an
    invalid time window and a tear-off that does not verify: the signed set is the Python flow's
    (resolve.commit_input_states gated on the verification), every signature is the model's and verifies."""
    import commit_log_worker as W
    from corda_amd import resolve as R
    kid, scheme, d, pub = keys[8]
    assert scheme == 3
    ftxs = _pmt_ok_cases()[:40]
    n = len(ftxs)
    assert n == 40
    leaves, toks, root = ftxs[9]
    ftxs[9] = (leaves, toks, bytes([root[0] ^ 1]) + root[1:])
    now, tol = 10**18, 10**9
    inputs = [[W.ref(2 * t), W.ref(2 * t + 1)] for t in range(n)]
    for t in (4, 17, 30):
        inputs[t] = [W.ref(2 * (t - 1)), W.ref(500 + t)]  # spends an input of the transaction before it
    inputs[31] = [W.ref(2 * 9)]                            # the unverified one committed nothing: no conflict
    windows = [None] * n
    windows[12] = (now + tol + 1, None)
    windows[13] = (now - 5, now + 5)
    callers = [7 + t % 3 for t in range(n)]
    ids = [f[2] for f in ftxs]
    verified = [1 if t == 9 else 0 for t in range(n)]
    flow_status, flow_committed, _, _ = R.commit_input_states(
        {}, [(ids[t], callers[t], inputs[t], windows[t]) for t in range(n)], now, tol, gate=verified)
    lid = engine.commit_log_create(10)
    try:
        answers, rows = R.notarise_filtered_transactions(engine, lid, ftxs, inputs, windows, callers, kid, now, tol)
    finally:
        engine.commit_log_destroy(lid)
    signed = [t for t in range(n) if isinstance(answers[t], bytes)]
    assert signed == [t for t in range(n) if flow_status[t] == OK] and len(signed) == 35
    assert {t: answers[t].kind for t in range(n) if t not in signed} == {
        4: "Conflict", 17: "Conflict", 30: "Conflict", 9: "TransactionInvalid", 12: "TimeWindowInvalid"}
    for t in signed:
        der = answers[t]
        assert der == M.sign(M.R1, d, ids[t]), t
        assert oracle.oracle_ecdsa_verify(3, pub, 65, der, len(der), ids[t], 32) == 0, t
    vst, _ = engine.verify_batch([3] * len(signed), [pub] * len(signed), [answers[t] for t in signed],
                                 [ids[t] for t in signed])
    assert not vst.any()
    assert len(rows) == sum(len(set(map(tuple, inputs[t]))) for t in range(n) if flow_committed[t])


# ---- 5. memory and replicas --------------------------------------------------------------------------
def test_signer_table_memory(engine):
    """The ECDSA signer's table is allocated by a context's first ECDSA add, counted in device_mem, kept by trim."""
    from corda_amd.engine import Engine
    engine.trim()
    with Engine(1) as eng:
        base = eng.device_mem(0)[0]
        ed, _ = eng.signer_add_ed25519(hashlib.sha256(b"mem-ed").digest())
        with_ed = eng.device_mem(0)[0]
        kid, st, pub = eng.signer_add_ecdsa(2, (5).to_bytes(32, "big"))
        assert st == OK and pub == M.public_key(M.K1, 5)
        with_ec = eng.device_mem(0)[0]
        assert with_ec - with_ed == SIGNTAB_BYTES and with_ed > base
        eng.signer_add_ecdsa(3, (6).to_bytes(32, "big"))
        assert eng.device_mem(0)[0] == with_ec  # one table, both curves, however many keys
        eng.ecdsa_sign_batch([kid] * 70, [b"x" * 40] * 70)
        eng.trim()
        assert eng.device_mem(0)[0] == with_ec  # the stages went, the tables stayed
        sig, ln, st = eng.ecdsa_sign_batch([kid], [b"after trim"])
        assert st[0] == OK and rows_equal(sig, ln, 0, M.sign(M.K1, 5, b"after trim"))


def test_three_device_replicas(golden, monkeypatch):
    """The shard split and the per-device tables on a context of three Device objects
    (CORDAHIP_TEST_DEVICE_REPLICAS): every replica holds the same record; add and remove reach all of them."""
    from corda_amd.engine import Engine
    monkeypatch.setenv("CORDAHIP_TEST_DEVICE_REPLICAS", "3")
    cases = [c for c in golden["cases"] if len(c["msg_b"]) == 32]
    with Engine(1) as eng:
        assert eng.device_count() == 3
        kid = {}
        for c in cases:
            k = golden["keys"][c["key"]]
            if c["key"] not in kid:
                kid[c["key"]], st, pub = eng.signer_add_ecdsa(k["scheme"], k["d_int"].to_bytes(32, "big"))
                assert st == OK and pub == k["pub_b"]
        lanes = [cases[i % len(cases)] for i in range(200)]  # shards of 128 and 72 lanes, the third empty
        sig, ln, st = eng.ecdsa_sign_batch([kid[c["key"]] for c in lanes], [c["msg_b"] for c in lanes])
        assert not st.any() and all(rows_equal(sig, ln, i, c["sig_b"]) for i, c in enumerate(lanes))
        for dev in range(3):
            dsig, dln, dst, _ = device_sign(eng, [kid[c["key"]] for c in cases[:4]], [c["msg_b"] for c in cases[:4]],
                                            device=dev)
            assert not dst.any() and all(rows_equal(dsig, dln, i, c["sig_b"]) for i, c in enumerate(cases[:4])), dev
        gone = kid[cases[0]["key"]]
        eng.signer_remove(gone)
        for dev in range(3):
            dsig, dln, dst, _ = device_sign(eng, [gone], [cases[0]["msg_b"]], device=dev)
            assert dst[0] == UNKNOWN and rows_equal(dsig, dln, 0, None), dev
