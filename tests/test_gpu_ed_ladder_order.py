"""The Ed25519 ladder with a block's lanes handed to its four waves in
window-count order (ed25519_ladder.hip, ED_LADDER_ORDER) on the GPU: statuses
and verdict words, bit for bit, against the C oracle.

The corpus (1,024 lanes, signed with the oracle, eight keys) is seeded so that
the reordering moves lanes across waves: h = SHA-512(R || A || M) mod L from
hashlib and the big-integer model of the prep's choice
(tools/proto/half_scalar_windows.py) give each lane's window count, and the
first 257 lanes hold lanes of 64 windows, of 65, and at least three of 66 or
more. Lane 40 is the longest lane a search of 200,000 messages found under the
six-candidate rule (LONG_MSG: 69 windows). About a fifth of the lanes carry a
flipped bit in R, S or the key, so ok bits differ between neighbours and a
verdict word assembled from the wrong lanes would show. Batches of 1, 63, 64,
65, 255, 256, 257 and 513 lanes end inside a wave and inside a block; status
and verdict arrays are prefilled with junk. The same corpus goes once through a
routed call with four of the eight keys registered, so that the routed
instance of the ladder runs reordered over the other lanes.

Lanes of more than 80 windows (the selector stream's `high` branch) are no
longer reachable by a search over messages: that branch stays covered on the
host by tests/test_ed_sel_recode.py."""
import ctypes
import hashlib
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("half_scalar_windows",
                                               os.path.join(ROOT, "tools", "proto", "half_scalar_windows.py"))
hw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(hw)

N = 1024
NKEYS = 8
SEED = 2          # the first seed that meets test_corpus_spreads_window_counts (found on a CPU)
LONG_LANE = 40
LONG_MSG = 37654  # of 200,000 messages under key 0: 69 windows (32 lanes of 68, 3 of 69)
LONG_WINDOWS = 68


def _sign(oracle, seed, msg):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_sign(seed, msg, 32, pub, sig)
    return pub.raw, sig.raw


def key_seed(k):
    return hashlib.sha256(b"order-key-%d" % k).digest()


def lane_windows(pub, sig, msg):
    """the lane's window count by the model: only for lanes whose R and key are as signed"""
    h = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % hw.L
    return hw.windows(hw.choose(h))


def make_corpus(oracle, seed=SEED, n=N):
    """(pubs, sigs, msgs as lists of bytes, windows: the model's count or -1 for a lane whose R or key was changed)"""
    pubs, sigs, msgs, win = [], [], [], []
    for i in range(n):
        if i == LONG_LANE:
            msg = hashlib.sha256(b"order-long-%d" % LONG_MSG).digest()
        else:
            msg = hashlib.sha256(b"order-%d-%d" % (seed, i)).digest()
        pub, sig = _sign(oracle, key_seed(i % NKEYS), msg)
        w = lane_windows(pub, sig, msg)
        d = hashlib.sha256(b"order-flip-%d-%d" % (seed, i)).digest()
        if d[0] % 5 == 0 and i != LONG_LANE:
            what, pos, bit = d[1] % 3, d[2], 1 << (d[3] % 8)
            if what == 0:    # R
                sig = sig[:pos % 32] + bytes([sig[pos % 32] ^ bit]) + sig[pos % 32 + 1:]
                w = -1
            elif what == 1:  # S: h and the window count stay
                p = 32 + pos % 32
                sig = sig[:p] + bytes([sig[p] ^ bit]) + sig[p + 1:]
            else:            # the key
                pub = pub[:pos % 32] + bytes([pub[pos % 32] ^ bit]) + pub[pos % 32 + 1:]
                w = -1
        pubs.append(pub)
        sigs.append(sig)
        msgs.append(msg)
        win.append(w)
    return pubs, sigs, msgs, win


def spreads(win):
    """what the reordering needs of the first 257 lanes"""
    head = win[:257]
    return 64 in head and 65 in head and sum(w >= 66 for w in head) >= 3


@pytest.fixture(scope="module")
def corpus(oracle):
    """the corpus on the device and the oracle's statuses: computed once, never written"""
    import torch
    dev = torch.device("cuda:0")
    pubs, sigs, msgs, win = make_corpus(oracle)
    k, s, m = (np.frombuffer(b"".join(x), np.uint8).reshape(N, -1).copy() for x in (pubs, sigs, msgs))
    want = np.zeros(N, np.uint8)
    oracle.oracle_ed25519_verify_batch(N, k.ctypes.data, s.ctypes.data, m.ctypes.data, 32, want.ctypes.data, 8)
    want.setflags(write=False)
    t = tuple(torch.from_numpy(x).to(dev) for x in (k, s, m))
    return t, want, win, pubs


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
    words = np.zeros((n + 63) // 64, np.uint64)
    for i in np.nonzero(want == 0)[0]:
        words[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    assert np.array_equal(vd, words), np.nonzero(vd != words)[0][:20]  # whole words: no bit past the batch


def test_corpus_spreads_window_counts(corpus):
    _, want, win, _ = corpus
    assert spreads(win), sorted(win[:257])
    assert win[LONG_LANE] >= LONG_WINDOWS, win[LONG_LANE]
    bad = (want != 0).sum()
    assert 0.1 * N < bad < 0.3 * N and len(set(want.tolist())) >= 3
    # neighbours differ: no verdict word of the first blocks is all ones or all zeros
    ok = (want == 0)
    assert all(0 < ok[64 * q:64 * q + 64].sum() < 64 for q in range(9))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_batches_end_inside_waves_and_blocks(engine, corpus, n):
    (pubs, sigs, msgs), want, _, _ = corpus
    st, vd = _verify(engine, pubs[:n].contiguous(), sigs[:n].contiguous(), msgs[:n].contiguous())
    _check(st, vd, want[:n])


def test_whole_corpus(engine, corpus):
    (pubs, sigs, msgs), want, _, _ = corpus
    st, vd = _verify(engine, pubs, sigs, msgs)
    _check(st, vd, want)


def test_routed_instance(oracle, corpus):
    from corda_amd.engine import Engine
    (pubs, sigs, msgs), want, _, pub_bytes = corpus
    with Engine(1) as eng:
        reg = []
        for k in range(NKEYS // 2):
            pub, _ = _sign(oracle, key_seed(k), b"\0" * 32)
            kid, st = eng.vkey_add_ed25519(pub)
            assert st == 0
            reg.append(pub)
        keyed = sum(p in reg for p in pub_bytes)
        assert N // 3 < keyed < N // 2 and N - keyed > 256 + 64  # the routed ladder has more than a block
        eng.vkey_set_routing(True)
        before = eng.vkey_route_stats()
        st, vd = _verify(eng, pubs, sigs, msgs)
        after = eng.vkey_route_stats()
        eng.vkey_set_routing(False)
        assert (after[0] - before[0], after[1] - before[1]) == (keyed, N - keyed)
        _check(st, vd, want)
