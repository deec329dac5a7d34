"""The Ed25519 ladder's joint (A, R) window table on the GPU, dense device path,
status bytes and verdict words against oracle/c: lane counts around the wave
and block edges, inputs that make table entries the identity or a doubling
(R = +-A, small-order A and R), and the signed-tx path whose prep runs as two
launches (ed25519_prep_keys_kernel / ed25519_prep_msg_kernel)."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

from corda_amd.corpus import C2_MIX, L, NONCANONICAL_R, SMALL_ORDER_KEYS, make_c2_corpus

pytestmark = pytest.mark.gpu

LANE_COUNTS = [1, 63, 64, 65, 257]


def _oracle_status(oracle, keys, sigs, msgs):
    keys, sigs, msgs = (np.ascontiguousarray(x, np.uint8) for x in (keys, sigs, msgs))
    n = keys.shape[0]
    out = np.zeros(n, np.uint8)
    oracle.oracle_ed25519_verify_batch(n, keys.ctypes.data, sigs.ctypes.data, msgs.ctypes.data, 32,
                                       out.ctypes.data, 4)
    return out


def _verify_device(engine, keys, sigs, msgs):
    """(status[n], verdict words[(n + 63) // 64]) of the dense device path"""
    import torch
    dev = torch.device("cuda:0")
    n = keys.shape[0]
    tk, ts, tm = (torch.from_numpy(np.array(x, np.uint8)).to(dev) for x in (keys, sigs, msgs))
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    vd = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    engine.ed25519_verify_device(tk, ts, tm, st, vd, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st.cpu().numpy(), vd.cpu().numpy().view(np.uint64)


def _check(got, verdict, want):
    assert np.array_equal(got, want), [(int(i), int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0][:20]]
    n = len(want)
    words = np.zeros((n + 63) // 64, np.uint64)
    for i in np.nonzero(want == 0)[0]:
        words[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    assert np.array_equal(verdict, words)


@pytest.fixture(scope="module")
def c2_corpus(engine, oracle):
    """257 seeded valid tuples with the C2 corruption catalogue at 20 %, and the oracle's statuses"""
    import torch
    dev = torch.device("cuda:0")
    pubs, sigs, msgs, _, cats = make_c2_corpus(engine, max(LANE_COUNTS), 20261019, dev, corrupt_frac=0.2)
    assert all(cats[name].numel() > 0 for name, _ in C2_MIX), {k: v.numel() for k, v in cats.items()}
    k, s, m = (t.cpu().numpy() for t in (pubs, sigs, msgs))
    return k, s, m, _oracle_status(oracle, k, s, m)


@pytest.mark.parametrize("n", LANE_COUNTS)
def test_lane_counts_vs_oracle(engine, c2_corpus, n):
    k, s, m, want = c2_corpus
    # the last n lanes for the small counts too: the corrupted lanes are spread over the corpus
    for lo in sorted({0, len(want) - n}):
        got, verdict = _verify_device(engine, k[lo:lo + n], s[lo:lo + n], m[lo:lo + n])
        _check(got, verdict, want[lo:lo + n])
    if n == len(want):
        assert 0 < (want != 0).sum() < n and (want == 0).sum() > n // 2


def _clamped_scalar(seed: bytes) -> int:
    h = bytearray(hashlib.sha512(seed).digest()[:32])
    h[0] &= 248
    h[31] &= 63
    h[31] |= 64
    return int.from_bytes(h, "little")


def _adversarial(engine):
    """64 lanes whose joint table holds the identity or a doubling where honest lanes hold
    a generic sum. Returns keys, sigs, msgs and the number of leading lanes that are valid."""
    import torch
    dev = torch.device("cuda:0")
    nk = 8
    seeds = np.frombuffer(b"".join(hashlib.sha256(b"joint-seed-%d" % i).digest() for i in range(nk)), np.uint8)
    seeds = seeds.reshape(nk, 32).copy()
    msgs8 = np.frombuffer(b"".join(hashlib.sha256(b"joint-msg-%d" % i).digest() for i in range(nk)), np.uint8)
    msgs8 = msgs8.reshape(nk, 32).copy()
    tp = torch.empty((nk, 32), dtype=torch.uint8, device=dev)
    tg = torch.empty((nk, 64), dtype=torch.uint8, device=dev)
    engine.ed25519_sign_device(torch.from_numpy(seeds).to(dev), torch.from_numpy(msgs8).to(dev), tp, tg)
    torch.cuda.synchronize()
    pubs, honest = tp.cpu().numpy(), tg.cpu().numpy()
    rows = []
    # R = A (r = a: S = (h + 1) a) and R = -A (r = -a: S = (h - 1) a), valid
    for sign in (1, -1):
        for i in range(nk):
            A, M = pubs[i].tobytes(), msgs8[i].tobytes()
            R = A if sign > 0 else A[:31] + bytes([A[31] ^ 0x80])
            h = int.from_bytes(hashlib.sha512(R + A + M).digest(), "little") % L
            S = (h + sign) * _clamped_scalar(seeds[i].tobytes()) % L
            rows.append((A, R + S.to_bytes(32, "little"), M))
    n_valid = len(rows)
    # the same tuples with one bit of S flipped
    for j, (A, sig, M) in enumerate(rows[:n_valid]):
        bit = (37 * j + 5) % 252
        s = bytearray(sig)
        s[32 + bit // 8] ^= 1 << (bit % 8)
        rows.append((A, bytes(s), M))
    so = [bytes.fromhex(x) for x in SMALL_ORDER_KEYS]
    ncr = [bytes.fromhex(x) for x in NONCANONICAL_R]
    zero_s = bytes(32)
    for i in range(nk):
        M = msgs8[i].tobytes()
        # small-order A under an honest signature's R and S
        rows.append((so[i], honest[i].tobytes(), M))
        # A = R small-order: with S = 0 the check reads -[h]A == A
        rows.append((so[i], so[i] + zero_s, M))
        # honest A, non-canonical R
        rows.append((pubs[i].tobytes(), ncr[(5 * i) % len(ncr)] + honest[i, 32:].tobytes(), M))
        # small-order A, small-order R != A, honest S
        rows.append((so[i], so[(i + 3) % 8] + honest[i, 32:].tobytes(), M))
    assert len(rows) == 64
    keys = np.frombuffer(b"".join(r[0] for r in rows), np.uint8).reshape(-1, 32)
    sigs = np.frombuffer(b"".join(r[1] for r in rows), np.uint8).reshape(-1, 64)
    msgs = np.frombuffer(b"".join(r[2] for r in rows), np.uint8).reshape(-1, 32)
    return keys, sigs, msgs, n_valid


def test_adversarial_table_inputs(engine, oracle):
    keys, sigs, msgs, n_valid = _adversarial(engine)
    want = _oracle_status(oracle, keys, sigs, msgs)
    # R = +-A with the matching S verifies; one flipped bit of S does not
    assert (want[:n_valid] == 0).all(), want[:n_valid]
    assert (want[n_valid:2 * n_valid] != 0).all(), want[n_valid:2 * n_valid]
    got, verdict = _verify_device(engine, keys, sigs, msgs)
    assert (got[:n_valid] == 0).all(), got[:n_valid]
    _check(got, verdict, want)


def test_signed_tx_split_prep(engine, oracle):
    """65 transactions through signed_tx_verify_ed25519_device: per-signature statuses,
    first bad signature and transaction status against the oracle"""
    import torch
    rng = random.Random(65)
    ntx = 65
    txs = [[bytes(rng.getrandbits(8) for _ in range(n)) for n in (120, 33, 64)] for _ in range(ntx)]
    ids, _ = engine.tx_ids(txs)
    nsig = [1 + t % 3 for t in range(ntx)]
    pub, sg = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    so = [bytes.fromhex(x) for x in SMALL_ORDER_KEYS]
    keys, sgs, owner = [], [], []
    for t in range(ntx):
        for k in range(nsig[t]):
            oracle.oracle_ed25519_sign(hashlib.sha256(b"stx%d" % ((3 * t + k) % 20)).digest(), ids[t].tobytes(), 32,
                                       pub, sg)
            p, s = pub.raw, sg.raw
            if t % 8 == 3 and k == nsig[t] - 1:
                s = s[:40] + bytes([s[40] ^ 4]) + s[41:]
            elif t % 8 == 5 and k == 0:
                p = so[t % 8]
            elif t % 8 == 7 and k == 0:
                s = p[:31] + bytes([p[31] ^ 0x80]) + s[32:]  # R = -A under a foreign S
            keys.append(p)
            sgs.append(s)
            owner.append(t)
    k_np = np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32)
    s_np = np.frombuffer(b"".join(sgs), np.uint8).reshape(-1, 64)
    want = _oracle_status(oracle, k_np, s_np, ids[owner])
    assert 0 < (want != 0).sum() < len(want)
    dev = torch.device("cuda:0")
    leaves = [x for tx in txs for x in tx]
    lb = torch.tensor(np.frombuffer(b"".join(leaves), np.uint8), device=dev)
    lo = torch.tensor(np.concatenate([[0], np.cumsum([len(x) for x in leaves])]).astype(np.int64), device=dev)
    tlo = torch.tensor(np.arange(0, 3 * ntx + 1, 3, dtype=np.int64), device=dev)
    sig_off = np.concatenate([[0], np.cumsum(nsig)]).astype(np.int64)
    tso = torch.tensor(sig_off, device=dev)
    txid = torch.empty((ntx, 32), dtype=torch.uint8, device=dev)
    tst = torch.empty(ntx, dtype=torch.uint8, device=dev)
    fb = torch.empty(ntx, dtype=torch.int64, device=dev)
    sst = torch.empty(len(keys), dtype=torch.uint8, device=dev)
    engine.signed_tx_verify_ed25519_device(lb, lo, tlo, tso, torch.from_numpy(k_np.copy()).to(dev),
                                           torch.from_numpy(s_np.copy()).to(dev), txid, tst, fb, sst)
    torch.cuda.synchronize()
    assert np.array_equal(txid.cpu().numpy(), ids)
    got = sst.cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:20]
    want_fb, want_tst = [], []
    for t in range(ntx):
        bad = np.nonzero(want[sig_off[t]:sig_off[t + 1]] != 0)[0]
        want_fb.append(int(bad[0]) if len(bad) else -1)
        want_tst.append(int(want[sig_off[t] + bad[0]]) if len(bad) else 0)
    assert list(fb.cpu().numpy()) == want_fb
    assert list(tst.cpu().numpy()) == want_tst
