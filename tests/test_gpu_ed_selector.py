"""The Ed25519 ladder fed by the prep's selector stream (ed25519_sel.hpp) on the
GPU, against the golden catalogue and the C oracle, status bytes and verdict
words both: batches that end inside a wave and inside a block (1, 63, 64, 65,
257, 1000 lanes), a corrupt_c2 corpus of 4,096 lanes in one launch pair, the
same corpus three times over in a context whose 64 MiB budget splits it into
two chunks (9,408 + 2,880 lanes), and one signed-tx call of 200 transactions,
whose records go through the split prep (keys, then messages)."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ED = 4
N = 4096


@pytest.fixture(scope="module")
def c2(engine, oracle):
    """(pubs, sigs, msgs) on the device and the oracle's statuses: computed once, never written"""
    import torch
    from corda_amd.corpus import make_c2_corpus
    dev = torch.device("cuda:0")
    # a quarter of the lanes carry one of the catalogue's corruptions
    pubs, sigs, msgs, exp, _ = make_c2_corpus(engine, N, 0xC0DA1401, dev, corrupt_frac=0.25)
    k, s, m = (np.ascontiguousarray(x.cpu().numpy()) for x in (pubs, sigs, msgs))
    want = np.zeros(N, np.uint8)
    oracle.oracle_ed25519_verify_batch(N, k.ctypes.data, s.ctypes.data, m.ctypes.data, 32, want.ctypes.data, 8)
    want.setflags(write=False)
    known = exp.cpu().numpy() >= 0
    assert np.array_equal(want[known], exp.cpu().numpy()[known].astype(np.uint8))  # construction and oracle agree
    assert 0.6 * N < (want == 0).sum() < 0.9 * N and len(set(want.tolist())) >= 3
    return pubs, sigs, msgs, want


def _verify(eng, pubs, sigs, msgs):
    import torch
    n = pubs.shape[0]
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=pubs.device)
    vd = torch.full(((n + 63) // 64,), 0x5A5A5A5A, dtype=torch.int64, device=pubs.device)
    eng.ed25519_verify_device(pubs, sigs, msgs, st, vd, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st.cpu().numpy(), vd.cpu().numpy().view(np.uint64)


def _check(st, vd, want):
    n = len(want)
    assert np.array_equal(st, want), np.nonzero(st != want)[0][:20]
    bits = (vd[np.arange(n) // 64] >> (np.arange(n) % 64).astype(np.uint64)) & np.uint64(1)
    assert np.array_equal(bits.astype(bool), want == 0)


def test_golden_catalogue(engine, ed_vectors):
    import torch
    dev = torch.device("cuda:0")
    vs = [v for v in ed_vectors if len(v["pub"]) == 32 and len(v["sig"]) == 64 and len(v["msg"]) == 32]
    assert len(vs) > 64
    up = lambda f, w: torch.from_numpy(np.frombuffer(b"".join(v[f] for v in vs), np.uint8).reshape(-1, w).copy()).to(dev)  # noqa: E731
    st, vd = _verify(engine, up("pub", 32), up("sig", 64), up("msg", 32))
    _check(st, vd, np.array([v["status"] for v in vs], np.uint8))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_partial_waves_and_blocks(engine, c2, n):
    pubs, sigs, msgs, want = c2
    # a slice that starts inside the corpus, so that every size sees corrupted lanes
    lo = 1500
    st, vd = _verify(engine, pubs[lo:lo + n].contiguous(), sigs[lo:lo + n].contiguous(), msgs[lo:lo + n].contiguous())
    _check(st, vd, want[lo:lo + n])


def test_corpus_in_one_launch_pair(engine, c2):
    pubs, sigs, msgs, want = c2
    st, vd = _verify(engine, pubs, sigs, msgs)
    _check(st, vd, want)


def test_corpus_in_several_chunks(c2):
    import torch  # noqa: F401
    from corda_amd.engine import Engine
    pubs, sigs, msgs, want = c2
    old = os.environ.get("CORDAHIP_DEVICE_MEM_BUDGET")
    os.environ["CORDAHIP_DEVICE_MEM_BUDGET"] = "64M"  # 9,408 lanes of workspace
    try:
        eng = Engine(1)
    finally:
        if old is None:
            del os.environ["CORDAHIP_DEVICE_MEM_BUDGET"]
        else:
            os.environ["CORDAHIP_DEVICE_MEM_BUDGET"] = old
    try:
        assert eng.device_mem(0)[2] == 64 << 20
        st, vd = _verify(eng, pubs.repeat(3, 1), sigs.repeat(3, 1), msgs.repeat(3, 1))
        _check(st, vd, np.tile(want, 3))
    finally:
        eng.close()


def test_signed_tx_split_prep(engine, oracle):
    ntx = 200
    txs = [[bytes([t % 256, q]) * (35 + 25 * q) for q in range(4)] for t in range(ntx)]
    ids, _ = engine.tx_ids(txs)
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    sigs = []
    for t in range(ntx):
        per = []
        for q in range(1 + t % 3):
            oracle.oracle_ed25519_sign(hashlib.sha256(b"sel%d-%d" % (t, q)).digest(), ids[t].tobytes(), 32, pub, sig)
            per.append((ED, pub.raw, sig.raw))
        if t % 7 == 2:  # a flipped bit in R or S of the last signature
            s = bytearray(per[-1][2])
            s[(t * 5) % 64] ^= 1 << (t % 8)
            per[-1] = (ED, per[-1][1], bytes(s))
        if t % 31 == 5:  # and a key that is another transaction's
            per[0] = (ED, sigs[t - 1][0][1], per[0][2])
        sigs.append(per)
    flat = [(x[1], x[2], ids[t].tobytes()) for t, per in enumerate(sigs) for x in per]
    n = len(flat)
    k, s, m = (np.frombuffer(b"".join(f[i] for f in flat), np.uint8).copy() for i in range(3))
    want = np.zeros(n, np.uint8)
    oracle.oracle_ed25519_verify_batch(n, k.ctypes.data, s.ctypes.data, m.ctypes.data, 32, want.ctypes.data, 8)
    assert 0 < (want != 0).sum() < n // 3
    got_ids, tx_status, first_bad, sig_status = engine.signed_tx_verify(txs, sigs)
    assert np.array_equal(got_ids, ids)
    assert np.array_equal(sig_status, want), np.nonzero(sig_status != want)[0][:20]
    off = np.cumsum([0] + [len(per) for per in sigs])
    for t in range(ntx):
        bad = np.nonzero(want[off[t]:off[t + 1]])[0]
        assert (tx_status[t] != 0) == (len(bad) > 0), t
        assert first_bad[t] == (bad[0] if len(bad) else -1), (t, first_bad[t], bad)
