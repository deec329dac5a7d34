"""Ed25519 batch signing with registered keys on the GPU (K11: cordahip_signer_add_ed25519,
cordahip_sign, cordahip_sign_submit, cordahip_ed25519_sign_keyed_device) against
tests/golden/ed25519_sign_vectors.json and the C oracle's oracle_ed25519_sign, byte for byte.
Outputs are prefilled with 0xA5, so a lane the library does not write shows."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from corda_amd import _lib
from corda_amd._lib import lib
from test_sign_vectors import load_sign_vectors

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OK, EMPTY, UNKNOWN, SKIPPED = _lib.OK, _lib.EMPTY, _lib.SIGN_UNKNOWN_KEY, _lib.SIGN_SKIPPED
GUARD = 64
KEYTAB_BYTES = (4096 * 32 + 32) * 4  # records + the expansion kernel's scratch


def csign(oracle, seed, msg):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_sign(seed, msg, len(msg), pub, sig)
    return pub.raw, sig.raw


@pytest.fixture(scope="module")
def vectors():
    return load_sign_vectors()


@pytest.fixture(scope="module")
def keys(engine, vectors):
    """The golden keys registered on the session engine: [(key_id, seed, pub)]."""
    out = []
    for k in vectors[0]:
        kid, pub = engine.signer_add_ed25519(k["seed"])
        assert pub == k["pub"], k["name"]
        out.append((kid, k["seed"], k["pub"]))
    assert len({k[0] for k in out}) == len(out)
    yield out
    for kid, _, _ in out:
        engine.signer_remove(kid)


class HostBatch:
    """cordahip_sign_batch arrays with guard bytes around sig and status, everything 0xA5."""

    def __init__(self, ids, msgs, gate=None):
        self.n = n = len(msgs)
        self.ids = np.asarray(ids, np.uint32)
        self.off = np.zeros(n + 1, np.uint64)
        self.off[1:] = np.cumsum([len(m) for m in msgs])
        self.msg = np.frombuffer(b"".join(msgs) or b"\0", np.uint8).copy()
        self.gate = None if gate is None else np.asarray(gate, np.uint8)
        self.sig_buf = np.full(GUARD + n * 64 + GUARD, 0xA5, np.uint8)
        self.st_buf = np.full(GUARD + n + GUARD, 0xA5, np.uint8)

    def batch(self, off=None, msg_bytes=None):
        p = lambda a: a.ctypes.data  # noqa: E731
        return _lib.SignBatch(self.n, p(self.ids), p(self.msg), p(self.off if off is None else off),
                              p(self.gate) if self.gate is not None else None, p(self.sig_buf) + GUARD,
                              p(self.st_buf) + GUARD, int(self.off[self.n]) if msg_bytes is None else msg_bytes)

    @property
    def sig(self):
        return self.sig_buf[GUARD:GUARD + self.n * 64].reshape(self.n, 64)

    @property
    def st(self):
        return self.st_buf[GUARD:GUARD + self.n]

    def guards_intact(self):
        return all((b[:GUARD] == 0xA5).all() and (b[-GUARD:] == 0xA5).all() for b in (self.sig_buf, self.st_buf))


def device_sign(engine, ids, msgs, gate=None, device=0, stream=None):
    """Dense rows through the device call; returns (sigs[n, 64], status[n]) as numpy."""
    import torch
    dev = torch.device("cuda:0")
    n = len(ids)
    stream = stream or torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        t_ids = torch.from_numpy(np.asarray(ids, np.uint32).view(np.int32).copy()).to(dev)
        t_msg = torch.from_numpy(np.frombuffer(b"".join(msgs), np.uint8).reshape(n, -1).copy()).to(dev)
        t_gate = None if gate is None else torch.from_numpy(np.asarray(gate, np.uint8).copy()).to(dev)
        t_sig = torch.full((n, 64), 0xA5, dtype=torch.uint8, device=dev)
        t_st = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        engine.ed25519_sign_keyed_device(t_ids, t_msg, t_sig, t_st, gate=t_gate, device=device, stream=stream)
    stream.synchronize()
    return t_sig.cpu().numpy(), t_st.cpu().numpy(), (t_msg, t_sig)


def test_golden_vectors_all_three_forms(engine, vectors, keys):
    _, vecs = vectors
    ids = [keys[v["key"]][0] for v in vecs]
    msgs = [v["msg"] for v in vecs]
    want = np.frombuffer(b"".join(v["sig"] for v in vecs), np.uint8).reshape(-1, 64)
    hb = HostBatch(ids, msgs)
    assert lib().cordahip_sign(engine.ctx, ctypes.byref(hb.batch())) == 0
    assert not hb.st.any() and np.array_equal(hb.sig, want) and hb.guards_intact()
    sig, st = engine.sign_batch(ids, msgs, async_=True).wait()
    assert not st.any() and np.array_equal(sig, want)
    for n in sorted({len(m) for m in msgs}):  # the device call takes dense rows: one call per length
        sel = [i for i, m in enumerate(msgs) if len(m) == n]
        sig, st, _ = device_sign(engine, [ids[i] for i in sel], [msgs[i] for i in sel])
        assert not st.any() and np.array_equal(sig, want[sel]), n


@pytest.fixture(scope="module")
def thousand(oracle, keys):
    """1,000 lanes, 5 keys interleaved, 32-byte messages, signed by the C oracle (once)."""
    n = 1000
    ids = [keys[i % 5][0] for i in range(n)]
    msgs = [hashlib.sha256(b"sign-lane-%d" % i).digest() for i in range(n)]
    sigs = np.frombuffer(b"".join(csign(oracle, keys[i % 5][1], msgs[i])[1] for i in range(n)), np.uint8)
    return ids, msgs, sigs.reshape(n, 64), [keys[i % 5][2] for i in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_lane_counts(engine, thousand, n):
    import torch
    ids, msgs, want, pubs = (x[:n] for x in thousand)
    sig, st, (t_msg, t_sig) = device_sign(engine, ids, msgs)
    assert not st.any()
    bad = [i for i in range(n) if not np.array_equal(sig[i], want[i])]
    assert not bad, bad[:10]
    hsig, hst = engine.sign_batch(ids, msgs)
    assert not hst.any() and np.array_equal(hsig, want)
    # what was signed verifies: the same rows through K1
    dev = t_sig.device
    t_pub = torch.from_numpy(np.frombuffer(b"".join(pubs), np.uint8).reshape(n, 32).copy()).to(dev)
    vst = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    engine.ed25519_verify_device(t_pub, t_sig, t_msg, vst, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert not vst.cpu().numpy().any()


def test_mixed_statuses_and_precedence(engine, oracle, keys):
    seed_a, seed_b = (hashlib.sha256(b"sign-mixed-%d" % i).digest() for i in range(2))
    removed, _ = engine.signer_add_ed25519(seed_a)
    engine.signer_remove(removed)
    assert lib().cordahip_signer_remove(engine.ctx, removed) == _lib.ERR_INVALID_ARG  # not live any more
    reused, pub_b = engine.signer_add_ed25519(seed_b)  # takes the freed slot under a new id
    assert reused != removed and (reused & 4095) == (removed & 4095)
    never = 4095 | (77 << 12)
    good, gseed = keys[0][0], keys[0][1]
    m = [hashlib.sha256(b"mixed-%d" % i).digest() for i in range(16)]
    lanes = [  # (key id, message, gate, expected status, seed of the expected signature)
        (good, m[0], 0, OK, gseed),
        (good, m[1], 1, SKIPPED, None),             # gated
        (good, m[2], 0, OK, gseed),
        (never, m[3], 0, UNKNOWN, None),            # an id no add ever returned
        (removed, m[4], 0, UNKNOWN, None),          # removed, its slot re-added since
        (reused, m[5], 0, OK, seed_b),              # the key that took the slot
        (good, b"", 0, EMPTY, None),                # empty message
        (good, m[7] + m[8], 0, OK, gseed),          # 64 bytes, right after an empty one
        (never, m[9], 7, SKIPPED, None),            # gated and unknown: SKIPPED first
        (good, b"", 1, SKIPPED, None),              # gated and empty
        (removed, b"", 0, UNKNOWN, None),           # unknown and empty: UNKNOWN_KEY before EMPTY
        (never, b"", 255, SKIPPED, None),           # all three
        (good, m[12], 0, OK, gseed),
    ]
    hb = HostBatch([x[0] for x in lanes], [x[1] for x in lanes], [x[2] for x in lanes])
    assert lib().cordahip_sign(engine.ctx, ctypes.byref(hb.batch())) == 0
    assert [int(s) for s in hb.st] == [x[3] for x in lanes]
    for i, (_, msg, _, st, seed) in enumerate(lanes):
        want = csign(oracle, seed, msg)[1] if st == OK else bytes(64)
        assert hb.sig[i].tobytes() == want, i
    assert hb.guards_intact()
    assert csign(oracle, seed_b, m[5])[0] == pub_b
    # the same through the device call (dense 32-byte rows, so no empty lanes)
    dl = [x for x in lanes if len(x[1]) == 32]
    sig, st, _ = device_sign(engine, [x[0] for x in dl], [x[1] for x in dl], [x[2] for x in dl])
    assert [int(s) for s in st] == [x[3] for x in dl]
    for i, (_, msg, _, s, seed) in enumerate(dl):
        assert sig[i].tobytes() == (csign(oracle, seed, msg)[1] if s == OK else bytes(64)), i
    # ungated: the NULL gate pointer
    sig, st = engine.sign_batch([good, never], [m[0], m[1]])
    assert [int(s) for s in st] == [OK, UNKNOWN] and sig[0].tobytes() == csign(oracle, gseed, m[0])[1]
    engine.signer_remove(reused)
    sig, st = engine.sign_batch([reused, good], [m[5], m[0]])
    assert [int(s) for s in st] == [UNKNOWN, OK] and not sig[0].any()


def _pmt_ok_cases():
    cases = json.load(open(os.path.join(HERE, "golden", "pmt_vectors.json")))["cases"]
    out = []
    for c in cases:
        if c["status"] == 0:
            out.append(([bytes.fromhex(x) for x in c["leaves"]],
                        [(t, bytes.fromhex(h) if h else None) for t, h in c["tokens"]], bytes.fromhex(c["root"])))
    return out


def test_gate_from_filtered_tx_verify(engine, oracle, keys):
    """Verify the tear-offs, then sign only what verified: the statuses of a real
    filtered_tx_verify call gate the device signer on one stream."""
    import torch
    from corda_amd import resolve as R
    ftxs = _pmt_ok_cases()
    assert len(ftxs) >= 4
    victim = len(ftxs) // 2
    leaves, toks, root = ftxs[victim]
    ftxs[victim] = (leaves, toks, bytes([root[0] ^ 1]) + root[1:])  # a root the tree does not hash to
    kid, seed, _ = keys[1]
    status = engine.filtered_tx_verify(ftxs)
    assert [int(s) != 0 for s in status] == [t == victim for t in range(len(ftxs))]
    stream = torch.cuda.Stream()
    sig, st, _ = device_sign(engine, [kid] * len(ftxs), [f[2] for f in ftxs], gate=status, stream=stream)
    for t, f in enumerate(ftxs):
        if t == victim:
            assert st[t] == SKIPPED and not sig[t].any()
        else:
            assert st[t] == OK and sig[t].tobytes() == csign(oracle, seed, f[2])[1]
            assert oracle.oracle_ed25519_verify(keys[1][2], 32, sig[t].tobytes(), 64, f[2], 32) == 0
    tx_status, sigs = R.verify_and_sign_filtered_transactions(engine, ftxs, kid)
    assert tx_status == [int(s) for s in status]
    assert sigs == [None if t == victim else sig[t].tobytes() for t in range(len(ftxs))]
    assert R.verify_and_sign_filtered_transactions(engine, [], kid) == ([], [])
    with pytest.raises(R.NoSuchElementException):
        R.verify_and_sign_filtered_transactions(engine, ftxs, 4095 | (99 << 12))


def test_small_chunks_two_tickets(engine, oracle, keys, monkeypatch):
    """CORDAHIP_HOST_CHUNK=256: 1,000 lanes of mixed lengths run as four chunks (dense
    32-byte ones and CSR ones), two batches in flight at once."""
    monkeypatch.setenv("CORDAHIP_HOST_CHUNK", "256")
    n = 1000
    lens = [32 if i < 300 else (0, 1, 31, 32, 33, 111, 112, 128, 240)[i % 9] for i in range(n)]
    batches = []
    for b in range(2):
        ids = [keys[(i + b) % len(keys)][0] for i in range(n)]
        msgs = [hashlib.shake_256(b"chunk-%d-%d" % (b, i)).digest(lens[i]) for i in range(n)]
        batches.append((ids, msgs, engine.sign_batch(ids, msgs, async_=True)))
    for b, (ids, msgs, ticket) in enumerate(batches):
        sig, st = ticket.wait()
        assert [int(s) for s in st] == [OK if l else EMPTY for l in lens]
        for i in range(0, n, 3):
            want = csign(oracle, keys[(i + b) % len(keys)][1], msgs[i])[1] if lens[i] else bytes(64)
            assert sig[i].tobytes() == want, (b, i, lens[i])


@pytest.fixture(scope="module")
def three_chunks(oracle, keys):
    """130 lanes for CORDAHIP_HOST_CHUNK=64, signed by the C oracle once: chunk 0 all 32-byte
    messages (dense rows), chunk 1 mixed lengths with 0- and 33-byte messages (CSR: the offset and
    length buffers are first needed in the middle of the call), chunk 2 a 2-lane tail."""
    lens = [32] * 64 + [(0, 33, 32, 1, 31, 64, 100)[i % 7] for i in range(64)] + [32, 32]
    n = len(lens)
    msgs = [hashlib.shake_256(b"sign-3chunk-%d" % i).digest(lens[i]) for i in range(n)]
    ids = [keys[i % len(keys)][0] for i in range(n)]
    want = [csign(oracle, keys[i % len(keys)][1], msgs[i])[1] if lens[i] else bytes(64) for i in range(n)]
    return ids, msgs, lens, want


@pytest.mark.parametrize("gated", [False, True])
def test_three_chunks_dense_csr_tail(engine, three_chunks, monkeypatch, gated):
    """The chunk loop's three shapes in one call, with a NULL gate and with gate bytes (a gated
    lane in each chunk, the tail's last lane among them)."""
    monkeypatch.setenv("CORDAHIP_HOST_CHUNK", "64")
    ids, msgs, lens, want = three_chunks
    n = len(lens)
    gate = [int(i % 9 == 3) * (1 + i % 255) for i in range(n)] if gated else None
    if gated:
        gate[129] = 1
        assert any(gate[:64]) and any(gate[64:128]) and gate[64] == 0  # lane 64 is empty and ungated
    hb = HostBatch(ids, msgs, gate)
    assert lib().cordahip_sign(engine.ctx, ctypes.byref(hb.batch())) == 0
    assert hb.guards_intact()
    skipped = [bool(gated and gate[i]) for i in range(n)]
    assert [int(s) for s in hb.st] == [SKIPPED if skipped[i] else OK if lens[i] else EMPTY for i in range(n)]
    bad = [i for i in range(n) if hb.sig[i].tobytes() != (bytes(64) if skipped[i] else want[i])]
    assert not bad, bad[:10]


def test_three_device_replicas(oracle, vectors, monkeypatch):
    """The shard split and the per-device key tables on a context of three Device objects
    (CORDAHIP_TEST_DEVICE_REPLICAS, read by cordahip_init): every replica holds the same
    record; add, remove and re-add reach all of them."""
    from corda_amd.engine import Engine
    monkeypatch.setenv("CORDAHIP_TEST_DEVICE_REPLICAS", "3")
    seeds = [k["seed"] for k in vectors[0][:3]]
    with Engine(1) as eng:
        assert eng.device_count() == 3
        ids = []
        for k in vectors[0][:3]:
            kid, pub = eng.signer_add_ed25519(k["seed"])
            assert pub == k["pub"]
            ids.append(kid)
        n = 300  # shards of 128, 128 and 44 lanes
        lane_ids = [ids[i % 3] for i in range(n)]
        msgs = [hashlib.sha256(b"replica-%d" % i).digest() for i in range(n)]
        want = [csign(oracle, seeds[i % 3], msgs[i])[1] for i in range(n)]
        sig, st = eng.sign_batch(lane_ids, msgs)
        assert not st.any() and [s.tobytes() for s in sig] == want
        for dev in range(3):
            dsig, dst, _ = device_sign(eng, lane_ids[:6], msgs[:6], device=dev)
            assert not dst.any() and [s.tobytes() for s in dsig] == want[:6], dev
        eng.signer_remove(ids[1])
        again, pub = eng.signer_add_ed25519(seeds[1])
        assert again != ids[1] and pub == vectors[0][1]["pub"]
        for dev in range(3):
            dsig, dst, _ = device_sign(eng, [ids[1], again, ids[0]], [msgs[1], msgs[1], msgs[0]], device=dev)
            assert [int(s) for s in dst] == [UNKNOWN, OK, OK], dev
            assert [s.tobytes() for s in dsig] == [bytes(64), want[1], want[0]], dev
        sig, st = eng.sign_batch([ids[1] if i % 3 == 1 else lane_ids[i] for i in range(n)], msgs)
        assert [int(s) for s in st] == [UNKNOWN if i % 3 == 1 else OK for i in range(n)]


@pytest.mark.parametrize("submit", [False, True])
def test_bad_msg_off_is_invalid_arg(engine, oracle, keys, submit):
    msgs = [hashlib.sha256(b"bad-off-%d" % i).digest()[:8 + i] for i in range(12)]
    hb = HostBatch([keys[0][0]] * 12, msgs)

    def run(batch):
        if not submit:
            return lib().cordahip_sign(engine.ctx, ctypes.byref(batch))
        t = ctypes.c_uint64()
        rc = lib().cordahip_sign_submit(engine.ctx, ctypes.byref(batch), ctypes.byref(t))
        return rc if rc != 0 else lib().cordahip_wait(engine.ctx, t.value, -1)

    dec = hb.off.copy()
    dec[5] = dec[6] + 3  # decreasing
    past = hb.off.copy()
    past[12] += 1        # one byte past the message buffer
    for bad in (hb.batch(off=dec), hb.batch(off=past), hb.batch(msg_bytes=int(hb.off[12]) - 1)):
        assert run(bad) == _lib.ERR_INVALID_ARG
        assert (hb.sig_buf == 0xA5).all() and (hb.st_buf == 0xA5).all()  # nothing was written
    assert run(hb.batch()) == 0  # the context stays usable
    assert not hb.st.any() and hb.guards_intact()
    assert [s.tobytes() for s in hb.sig] == [csign(oracle, keys[0][1], m)[1] for m in msgs]


def test_key_table_memory(engine):
    """The key table is allocated by a context's first add, counted in device_mem and kept by trim."""
    from corda_amd.engine import Engine
    engine.trim()  # nothing of the session engine's left to release meanwhile
    with Engine(1) as eng:
        base = eng.device_mem(0)[0]
        kid, _ = eng.signer_add_ed25519(hashlib.sha256(b"mem-key").digest())
        with_table = eng.device_mem(0)[0]
        assert with_table - base == KEYTAB_BYTES
        eng.signer_add_ed25519(hashlib.sha256(b"mem-key-2").digest())
        assert eng.device_mem(0)[0] == with_table  # one table, however many keys
        eng.sign_batch([kid] * 70, [b"x" * 40] * 70)
        eng.trim()
        assert eng.device_mem(0)[0] == with_table  # the stages went, the table stayed
        sig, st = eng.sign_batch([kid], [b"after trim"])
        assert st[0] == OK and sig[0].any()
