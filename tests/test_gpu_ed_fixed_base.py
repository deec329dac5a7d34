"""The Ed25519 ladder's three shortened group operations on the GPU
(ed25519_ladder.hip): fixed-base windows of ED_B_BITS bits with fewer digits
over B' than over B, the top window loaded as the accumulator instead of added
to the identity (ED_LADDER_TOP_LOAD), and the verdict taken from the last
addition's E, F, H (ED_LADDER_LAST_EH). Everything is compared with the C
oracle on status bytes and verdict words, outputs prefilled with junk.

Corpus batches: a corrupt_c2 corpus of 4,096 lanes, a quarter of them
corrupted; 1, 63, 64, 65, 257 and 1000 lanes cut from inside it; three copies
of it in a context whose 64 MiB budget splits them into chunks; and the corpus
through a routed call with the keys of 40 lanes registered, so that the routed
instance of the ladder runs over the rest.

Extreme digits: e = c1 S mod L with c1 from the big-integer model of the prep's
choice (tools/proto/half_scalar_windows.py). A search of 200,000 messages
"fixed-base-<i>" under one oracle key, on a CPU, for lanes with a 20-bit
fixed-base digit of 0 or +-1 (below the top digit) or of magnitude >= 2^19 - 2
found 21; EXTREME bakes 13 of them in, among them both ends of the range
exactly: +2^19 (message 35707, digit 1) and -2^19 (60256, digit 8; 73301,
digit 7). The test derives the digits again and checks them against the list,
so the list cannot go stale unnoticed; at another width than 20 the lanes are
ordinary ones, and tests/test_ed_bdigits.py covers the extremes of every width
on the host.

Top window that is also a fixed-base window (the wave has no scalars of its
own, so it runs the minimum window count and the mixed additions that follow
the top window need T): 64 and 257 lanes that the prep decides, all of them,
with the catalogue's keys of status BAD_KEY (off the curve; categories
key_noncanonical_y and key_small_y); and 64 lanes with one valid lane among 63
of those. The catalogue's non-canonical keys that decode under the i2p rules run
the ladder like any key; they go through in test_catalogue_keys.

The largest window count on record: LONG_MSG of tests/test_gpu_ed_ladder_order.py
(69 windows by the model) in one wave with lanes of 64 windows, so that the top
windows of every other lane select the identity entry, (1, 1, 1, 0), which the
load turns into (0 : 2 : 2)."""
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

N = 4096
B_BITS, B_DIGITS = 20, 13
# (message index, digit position, digit) found by the search the docstring describes
EXTREME = [(4503, 5, 1), (199815, 2, -1), (119728, 3, 1), (29048, 9, 0), (44003, 7, 0),
           (35707, 1, 1 << 19), (60256, 8, -(1 << 19)), (73301, 7, -(1 << 19)),
           (16177, 9, -(1 << 19) + 1), (51403, 9, (1 << 19) - 1), (199747, 0, -(1 << 19) + 1),
           (45677, 9, (1 << 19) - 2), (56741, 5, -(1 << 19) + 2)]
EXTREME_KEY = hashlib.sha256(b"fixed-base-key-0").digest()
LONG_KEY = hashlib.sha256(b"order-key-0").digest()
LONG_MSG = 37654  # tests/test_gpu_ed_ladder_order.py: 69 windows by the model
LONG_WINDOWS = 68


def _sign(oracle, seed, msg):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_sign(seed, msg, 32, pub, sig)
    return pub.raw, sig.raw


def _model(pub, sig, msg):
    """(window count, fixed-base digits of width B_BITS) of a lane as signed, by the big-integer model"""
    h = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % hw.L
    c0, c1 = hw.choose(h)
    e = c1 * int.from_bytes(sig[32:], "little") % hw.L
    digits = []
    for t in range(B_DIGITS):
        v = ((e << 1) >> (B_BITS * t)) & ((2 << B_BITS) - 1)
        digits.append(((v + 1) >> 1) - ((v >> B_BITS) << B_BITS))
    assert sum(d << (B_BITS * t) for t, d in enumerate(digits)) == e
    return hw.windows((c0, c1)), digits


def _flip_s(sig, k):
    p = 32 + k % 31
    return sig[:p] + bytes([sig[p] ^ (1 << (k % 8))]) + sig[p + 1:]


def _oracle_status(oracle, lanes):
    n = len(lanes)
    k, s, m = (np.frombuffer(b"".join(x[i] for x in lanes), np.uint8).reshape(n, -1).copy() for i in range(3))
    want = np.zeros(n, np.uint8)
    oracle.oracle_ed25519_verify_batch(n, k.ctypes.data, s.ctypes.data, m.ctypes.data, 32, want.ctypes.data, 8)
    return (k, s, m), want


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


def _run_lanes(engine, oracle, lanes):
    import torch
    dev = torch.device("cuda:0")
    arrays, want = _oracle_status(oracle, lanes)
    st, vd = _verify(engine, *(torch.from_numpy(x).to(dev) for x in arrays))
    _check(st, vd, want)
    return want


@pytest.fixture(scope="module")
def c2(engine, oracle):
    """(pubs, sigs, msgs) on the device and the oracle's statuses: computed once, never written"""
    import torch
    from corda_amd.corpus import make_c2_corpus
    dev = torch.device("cuda:0")
    pubs, sigs, msgs, exp, _ = make_c2_corpus(engine, N, 0xC0DA2401, dev, corrupt_frac=0.25)
    k, s, m = (np.ascontiguousarray(x.cpu().numpy()) for x in (pubs, sigs, msgs))
    want = np.zeros(N, np.uint8)
    oracle.oracle_ed25519_verify_batch(N, k.ctypes.data, s.ctypes.data, m.ctypes.data, 32, want.ctypes.data, 8)
    want.setflags(write=False)
    known = exp.cpu().numpy() >= 0
    assert np.array_equal(want[known], exp.cpu().numpy()[known].astype(np.uint8))  # construction and oracle agree
    assert 0.6 * N < (want == 0).sum() < 0.9 * N and len(set(want.tolist())) >= 3
    return pubs, sigs, msgs, want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_batches_cut_from_inside_the_corpus(engine, c2, n):
    pubs, sigs, msgs, want = c2
    lo = 2047  # every size sees corrupted lanes; no batch starts on a wave of the corpus
    st, vd = _verify(engine, pubs[lo:lo + n].contiguous(), sigs[lo:lo + n].contiguous(), msgs[lo:lo + n].contiguous())
    _check(st, vd, want[lo:lo + n])
    assert n < 63 or (want[lo:lo + n] != 0).any()


def test_whole_corpus(engine, c2):
    pubs, sigs, msgs, want = c2
    st, vd = _verify(engine, pubs, sigs, msgs)
    _check(st, vd, want)


def test_corpus_in_several_chunks(c2):
    import torch  # noqa: F401
    from corda_amd.engine import Engine
    pubs, sigs, msgs, want = c2
    old = os.environ.get("CORDAHIP_DEVICE_MEM_BUDGET")
    os.environ["CORDAHIP_DEVICE_MEM_BUDGET"] = "64M"  # 9,408 lanes of workspace: 12,288 lanes are two chunks
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


def test_routed_instance(c2):
    from corda_amd.engine import Engine
    pubs, sigs, msgs, want = c2
    pub_bytes = [bytes(r) for r in pubs.cpu().numpy()]
    with Engine(1) as eng:
        reg = set()
        for i in np.nonzero(want == 0)[0][100:140]:  # 40 valid lanes' keys
            kid, st = eng.vkey_add_ed25519(pub_bytes[i])
            assert st == 0
            reg.add(pub_bytes[i])
        keyed = sum(p in reg for p in pub_bytes)
        assert 40 <= keyed < 64 and N - keyed > 256 + 64  # the routed ladder has more than a block
        eng.vkey_set_routing(True)
        before = eng.vkey_route_stats()
        st, vd = _verify(eng, pubs, sigs, msgs)
        after = eng.vkey_route_stats()
        eng.vkey_set_routing(False)
        assert (after[0] - before[0], after[1] - before[1]) == (keyed, N - keyed)
        _check(st, vd, want)


def test_extreme_fixed_base_digits(engine, oracle):
    lanes = []
    for k, (i, t, d) in enumerate(EXTREME):
        msg = hashlib.sha256(b"fixed-base-%d" % i).digest()
        pub, sig = _sign(oracle, EXTREME_KEY, msg)
        assert _model(pub, sig, msg)[1][t] == d, (i, t, d)
        # the extreme lane, a lane with another e on the same message (rejected), ordinary lanes
        lanes.append((pub, sig, msg))
        lanes.append((pub, _flip_s(sig, k), msg))
        for q in range(3):
            m2 = hashlib.sha256(b"fixed-base-plain-%d-%d" % (i, q)).digest()
            lanes.append(_sign(oracle, EXTREME_KEY, m2) + (m2,))
    assert len(lanes) == 65  # a full wave and one lane
    want = _run_lanes(engine, oracle, lanes)
    assert all(want[5 * k] == 0 and want[5 * k + 1] == 1 for k in range(len(EXTREME)))


def _decided(ed_vectors):
    vs = [v for v in ed_vectors if v["status"] == 3 and v["cat"] in ("key_noncanonical_y", "key_small_y")
          and len(v["pub"]) == 32 and len(v["sig"]) == 64 and len(v["msg"]) == 32]
    assert len(vs) == 28
    return [(v["pub"], v["sig"], v["msg"]) for v in vs]


@pytest.mark.parametrize("n", [64, 257])
def test_every_lane_decided_in_the_prep(engine, oracle, ed_vectors, n):
    dec = _decided(ed_vectors)
    want = _run_lanes(engine, oracle, [dec[i % len(dec)] for i in range(n)])
    assert (want == 3).all()


def test_one_valid_lane_among_decided_ones(engine, oracle, ed_vectors):
    dec = _decided(ed_vectors)
    valid = next((v["pub"], v["sig"], v["msg"]) for v in ed_vectors
                 if v["cat"] == "valid" and v["status"] == 0 and len(v["msg"]) == 32)
    lanes = [dec[i % len(dec)] for i in range(64)]
    lanes[37] = valid
    want = _run_lanes(engine, oracle, lanes)
    assert want[37] == 0 and (np.delete(want, 37) == 3).all()


def test_catalogue_keys(engine, oracle, ed_vectors):
    vs = [(v["pub"], v["sig"], v["msg"]) for v in ed_vectors
          if v["cat"].startswith("key_") and len(v["pub"]) == 32 and len(v["sig"]) == 64 and len(v["msg"]) == 32]
    want = _run_lanes(engine, oracle, vs)
    assert len(vs) > 64 and {0, 1, 3} <= set(want.tolist())


def test_longest_lane_among_64_window_lanes(engine, oracle):
    lanes, i = [], 0
    while len(lanes) < 64:
        msg = hashlib.sha256(b"fixed-base-w64-%d" % i).digest()
        pub, sig = _sign(oracle, LONG_KEY, msg)
        i += 1
        if _model(pub, sig, msg)[0] != 64:
            continue
        if len(lanes) % 9 == 4:  # S changed: c1 and the window count stay, the verdict does not
            sig = _flip_s(sig, i)
        lanes.append((pub, sig, msg))
    msg = hashlib.sha256(b"order-long-%d" % LONG_MSG).digest()
    pub, sig = _sign(oracle, LONG_KEY, msg)
    assert _model(pub, sig, msg)[0] >= LONG_WINDOWS
    lanes[21] = (pub, sig, msg)
    want = _run_lanes(engine, oracle, lanes)
    assert want[21] == 0 and (want != 0).sum() >= 6
