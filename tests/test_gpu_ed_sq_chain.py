"""The Ed25519 prep's square chains (ge25519.hpp fe_sqn_pair over fe_sqsq2, and
the 13-operand squarings) on the GPU, through ed25519_verify_device: status
bytes and verdict words against oracle/c at lane counts around the wave and
block edges. The decompression exponent z^(2^252 - 3) is where the chains run,
so the lanes hold what steers it: GPU-signed valid tuples whose keys and R take
both square-root branches (root as computed, root times sqrt(-1)), the corpus
module's non-canonical, off-curve and small-order encodings, and keys and R
with y in {0, 1, p - 1, p, 2^255 - 1} under both sign bits."""
import hashlib

import numpy as np
import pytest

from corda_amd.corpus import NONCANONICAL_KEYS, NONCANONICAL_R, OFF_CURVE_KEYS, P, SMALL_ORDER_KEYS

pytestmark = pytest.mark.gpu

LANE_COUNTS = [1, 63, 64, 65, 257, 1024]
N = max(LANE_COUNTS)
D = -121665 * pow(121666, -1, P) % P
EDGE_Y = [0, 1, P - 1, P, 2**255 - 1]


def sqrt_branch(enc: bytes):
    """How ge_frombytes finds x for the encoding's y (bit 255 ignored, y not
    reduced first): 0 = the candidate root u v^3 (u v^7)^((p-5)/8) itself,
    1 = the candidate times sqrt(-1), None = y is not on the curve."""
    y = int.from_bytes(enc, "little") & (2**255 - 1)
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    vxx = v * x * x % P
    if vxx == u:
        return 0
    return 1 if vxx == (P - u) % P else None


def _oracle_status(oracle, keys, sigs, msgs):
    keys, sigs, msgs = (np.ascontiguousarray(x, np.uint8) for x in (keys, sigs, msgs))
    n = keys.shape[0]
    out = np.zeros(n, np.uint8)
    oracle.oracle_ed25519_verify_batch(n, keys.ctypes.data, sigs.ctypes.data, msgs.ctypes.data, 32,
                                       out.ctypes.data, 4)
    return out


def _verify_device(engine, keys, sigs, msgs):
    import torch
    dev = torch.device("cuda:0")
    n = keys.shape[0]
    tk, ts, tm = (torch.from_numpy(np.array(x, np.uint8)).to(dev) for x in (keys, sigs, msgs))
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    vd = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    engine.ed25519_verify_device(tk, ts, tm, st, vd, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    return st.cpu().numpy(), vd.cpu().numpy().view(np.uint64)


def _special_rows():
    """(column, 32-byte encoding): the catalogue tables, then the edge y values"""
    rows = [("key", bytes.fromhex(x)) for x in NONCANONICAL_KEYS + OFF_CURVE_KEYS + SMALL_ORDER_KEYS]
    rows += [("r", bytes.fromhex(x)) for x in NONCANONICAL_R]
    for y in EDGE_Y:
        for sign in (0, 1):
            enc = (y | sign << 255).to_bytes(32, "little")
            rows += [("key", enc), ("r", enc)]
    return rows


@pytest.fixture(scope="module")
def lanes(engine, oracle):
    """1024 GPU-signed tuples; every third lane below 3 * len(specials) carries a
    special key or R in place of the honest one. Returns keys, sigs, msgs, the
    oracle's statuses and the mask of untouched lanes."""
    import torch
    dev = torch.device("cuda:0")
    seeds = np.frombuffer(b"".join(hashlib.sha256(b"sq-chain-seed-%d" % i).digest() for i in range(N)), np.uint8)
    msgs = np.frombuffer(b"".join(hashlib.sha256(b"sq-chain-msg-%d" % i).digest() for i in range(N)), np.uint8)
    seeds, msgs = seeds.reshape(N, 32).copy(), msgs.reshape(N, 32).copy()
    tp = torch.empty((N, 32), dtype=torch.uint8, device=dev)
    tg = torch.empty((N, 64), dtype=torch.uint8, device=dev)
    engine.ed25519_sign_device(torch.from_numpy(seeds).to(dev), torch.from_numpy(msgs).to(dev), tp, tg)
    torch.cuda.synchronize()
    keys, sigs = tp.cpu().numpy().copy(), tg.cpu().numpy().copy()
    honest = np.ones(N, bool)
    special = _special_rows()
    assert 3 * len(special) <= 257  # all of them within the 257-lane slice
    for s, (col, enc) in enumerate(special):
        lane = 3 * s + 2
        honest[lane] = False
        if col == "key":
            keys[lane] = np.frombuffer(enc, np.uint8)
        else:
            sigs[lane, :32] = np.frombuffer(enc, np.uint8)
    return keys, sigs, msgs, _oracle_status(oracle, keys, sigs, msgs), honest


def test_valid_lanes_take_both_root_branches(lanes):
    """among the first 256 honest lanes, each branch in at least a quarter, for A and for R"""
    keys, sigs, _, want, honest = lanes
    idx = np.nonzero(honest)[0][:256]
    assert len(idx) == 256 and (want[honest] == 0).all()
    for enc in (keys[idx], sigs[idx, :32]):
        br = [sqrt_branch(e.tobytes()) for e in enc]
        assert None not in br
        assert br.count(0) >= 64 and br.count(1) >= 64, (br.count(0), br.count(1))


def test_special_lanes_cover_every_decode_outcome(lanes):
    """the special encodings hold off-curve values and both branches, and the oracle rejects
    some and accepts none silently: a key that decodes leaves the verdict to the equation"""
    _, _, _, want, honest = lanes
    br = [sqrt_branch(enc) for _, enc in _special_rows()]
    assert br.count(None) >= len(OFF_CURVE_KEYS) and br.count(0) and br.count(1)
    assert (want[~honest] != 0).sum() >= len(OFF_CURVE_KEYS)
    assert len(set(want[~honest].tolist())) >= 2  # bad key and bad signature statuses


@pytest.mark.parametrize("n", LANE_COUNTS)
def test_lane_counts_vs_oracle(engine, lanes, n):
    keys, sigs, msgs, want, _ = lanes
    for lo in sorted({0, 2, N - n} if n == 1 else {0, N - n}):  # lane 2 is a special one
        got, verdict = _verify_device(engine, keys[lo:lo + n], sigs[lo:lo + n], msgs[lo:lo + n])
        w = want[lo:lo + n]
        assert np.array_equal(got, w), [(int(i), int(got[i]), int(w[i])) for i in np.nonzero(got != w)[0][:20]]
        words = np.zeros((n + 63) // 64, np.uint64)
        for i in np.nonzero(w == 0)[0]:
            words[i // 64] |= np.uint64(1) << np.uint64(i % 64)
        assert np.array_equal(verdict, words)
