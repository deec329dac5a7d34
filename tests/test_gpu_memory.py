"""The device-memory budget and the idle release (ABI 4: CORDAHIP_DEVICE_MEM_BUDGET,
cordahip_device_mem, cordahip_trim, CORDAHIP_IDLE_RELEASE_MS) on the GPU: a context
with a 64 MiB budget sizes its Ed25519 workspace at ~9.4 k lanes and its ECDSA
workspace at ~9 k slots, so C2-, C3- and c4h-shaped batches run in several launch
sets each; every result matches the construction and the C oracle on samples; the
bytes the library holds stay within the budget's workspaces plus the batch
buffers; cordahip_trim and the idle release give them back, and the context
verifies again afterwards. (Host process reference: the JVM node that hosts the
library, SignedTransaction.kt:95-100.)"""
import ctypes
import hashlib
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ED = 4
MIB = 1 << 20


@pytest.fixture(scope="module")
def small():
    import torch  # noqa: F401
    from corda_amd.engine import Engine
    old = {k: os.environ.get(k) for k in ("CORDAHIP_DEVICE_MEM_BUDGET", "CORDAHIP_IDLE_RELEASE_MS")}
    os.environ["CORDAHIP_DEVICE_MEM_BUDGET"] = "64M"
    os.environ["CORDAHIP_IDLE_RELEASE_MS"] = "400"
    try:
        eng = Engine(1)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    yield eng
    eng.close()


def test_budget_reported(small):
    in_use, peak, budget = small.device_mem(0)
    assert budget == 64 * MIB and peak >= in_use > 0


def test_c2_shape_in_several_launch_sets(small, oracle):
    import torch
    from corda_amd.corpus import make_c2_corpus
    dev = torch.device("cuda:0")
    n = 50_000  # > 9,408 lanes of workspace: 6 launch pairs
    pubs, sigs, msgs, exp, _ = make_c2_corpus(small, n, 0xC0DA0601, dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    base = small.device_mem(0)[0]
    small.ed25519_verify_device(pubs, sigs, msgs, st, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = st.cpu()
    known = exp.cpu() >= 0
    assert (got[known].to(torch.int16) == exp.cpu()[known]).all()
    k = np.ascontiguousarray(pubs[:4000].cpu().numpy())
    s = np.ascontiguousarray(sigs[:4000].cpu().numpy())
    m = np.ascontiguousarray(msgs[:4000].cpu().numpy())
    want = np.zeros(4000, np.uint8)
    oracle.oracle_ed25519_verify_batch(4000, k.ctypes.data, s.ctypes.data, m.ctypes.data, 32, want.ctypes.data, 4)
    assert np.array_equal(got[:4000].numpy(), want)
    in_use, peak, budget = small.device_mem(0)
    # the workspace the budget allows (45% of it), nothing batch-sized on the device path
    assert in_use - base <= budget * 45 // 100 + MIB


def test_c3_shape_in_several_launch_sets(small, oracle):
    import torch
    from corda_amd.corpus import make_c3_corpus
    dev = torch.device("cuda:0")
    n = 30_000  # > ~9 k ECDSA slots: 4 launch sets
    scheme, keys, key_len, sigs, sig_len, msgs, exp, _ = make_c3_corpus(small, n, 0xC0DA0602, dev)
    st = torch.empty(n, dtype=torch.uint8, device=dev)
    small.ecdsa_verify_device(scheme, keys, key_len, sigs, sig_len, msgs, st, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = st.cpu()
    known = exp.cpu() >= 0
    assert (got[known].to(torch.int16) == exp.cpu()[known]).all()
    idx = np.arange(0, n, 15)
    sch, K, KL, S, SL, M = (x.cpu().numpy()[idx] for x in (scheme, keys, key_len, sigs, sig_len, msgs))
    kb = np.ascontiguousarray(np.concatenate([K[i, :KL[i]] for i in range(len(idx))]))
    sb = np.ascontiguousarray(np.concatenate([S[i, :SL[i]] for i in range(len(idx))]))
    ko = np.zeros(len(idx) + 1, np.uint64)
    so = np.zeros(len(idx) + 1, np.uint64)
    ko[1:] = np.cumsum(KL.astype(np.uint64))
    so[1:] = np.cumsum(SL.astype(np.uint64))
    mo = np.arange(len(idx) + 1, dtype=np.uint64) * 32
    want = np.zeros(len(idx), np.uint8)
    Mc = np.ascontiguousarray(M)
    sch = np.ascontiguousarray(sch)
    oracle.oracle_ecdsa_verify_batch(len(idx), sch.ctypes.data, kb.ctypes.data, ko.ctypes.data, sb.ctypes.data,
                                     so.ctypes.data, Mc.ctypes.data, mo.ctypes.data, want.ctypes.data, 4)
    assert np.array_equal(got.numpy()[idx], want)


def _sign(oracle, seed, msg):
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    oracle.oracle_ed25519_sign(seed, msg, len(msg), pub, sig)
    return pub.raw, sig.raw


def test_c4h_shape_trim_and_idle_release(small, engine, oracle):
    ntx = 12_000
    txs = [[bytes([t % 256, q]) * (40 + 30 * q) for q in range(5)] for t in range(ntx)]
    ids, _ = engine.tx_ids(txs)
    sigs = []
    for t in range(ntx):
        per = [(ED,) + _sign(oracle, hashlib.sha256(b"m%d-%d" % (t, q)).digest(), ids[t].tobytes())
               for q in range(1 + t % 3)]
        if t % 11 == 4:
            per[-1] = (ED, per[-1][1], per[-1][2][:30] + bytes([per[-1][2][30] ^ 1]) + per[-1][2][31:])
        sigs.append(per)
    want = engine.signed_tx_verify(txs, sigs)  # the session context, default budget
    got = small.signed_tx_verify(txs, sigs)    # 64 MiB: every chunk in several launch pairs
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert (got[1] == 1).sum() == len(range(4, ntx, 11))
    before = small.device_mem(0)[0]
    small.trim()
    after = small.device_mem(0)[0]
    assert after < before
    # the idle release (400 ms here) after another call: the buffers go back by themselves
    got2 = small.signed_tx_verify(txs, sigs)
    assert all(np.array_equal(a, b) for a, b in zip(got2, want))
    grown = small.device_mem(0)[0]
    deadline = time.time() + 10
    while time.time() < deadline and small.device_mem(0)[0] >= grown:
        time.sleep(0.2)
    assert small.device_mem(0)[0] < grown
    got3 = small.signed_tx_verify(txs[:100], sigs[:100])  # and the context still verifies
    assert np.array_equal(got3[1], want[1][:100])


def test_component_slices_in_pieces(small, engine, oracle):
    """cordahip_txcomp_submit under the 64 MiB budget: the full encoder chain's leaf buffer
    is capped at a tenth of the budget (6.7 MB, ~300 cash-issue transactions' bound), so
    each id slice is encoded and hashed in pieces of whole transactions; ids, statuses and
    first_bad_sig equal the default context's and the oracle's ids"""
    from corda_amd import _lib
    from corda_amd.corpus import cash_issue_items
    rng = np.random.default_rng(61)
    ntx = 3000
    blob, items, _ = cash_issue_items(rng.integers(0, 256, (ntx, 32), dtype=np.uint8),
                                      rng.integers(0, 256, (ntx, 32), dtype=np.uint8), bytes(range(32)),
                                      rng.integers(1, 10**9, ntx), rng.integers(-2**63, 2**63 - 1, ntx))
    it = items.reshape(-1).copy()
    host_it = it.copy()
    host_it["data"] += np.uint64(blob.ctypes.data)
    hb, ho = _lib.kryo_encode_array(host_it)
    leaves = [[hb[int(ho[5 * t + j]):int(ho[5 * t + j + 1])].tobytes() for j in range(5)] for t in range(ntx)]
    ids_l, _ = engine.tx_ids(leaves)
    for t in range(0, ntx, 499):  # the oracle's ids on a sample
        want = ctypes.create_string_buffer(32)
        lb = np.frombuffer(b"".join(leaves[t]), np.uint8).copy()
        lo = np.zeros(6, np.uint64)
        lo[1:] = np.cumsum([len(x) for x in leaves[t]])
        assert oracle.oracle_tx_id(lb.ctypes.data, lo.ctypes.data, 5, want) == 0
        assert want.raw == ids_l[t].tobytes()
    sigs = []
    for t in range(ntx):
        pub, sg = _sign(oracle, hashlib.sha256(b"pc%d" % t).digest(), ids_l[t].tobytes())
        if t % 13 == 5:
            sg = sg[:7] + bytes([sg[7] ^ 2]) + sg[8:]
        sigs.append([(ED, pub, sg)] * (1 + t % 3))
    tio = np.arange(0, 5 * ntx + 1, 5, dtype=np.uint64)
    want = engine.signed_txcomp_verify_arrays(blob, it, tio, sigs)
    for _ in range(2):  # the first call on the small context runs the full chain
        got = small.signed_txcomp_verify_arrays(blob, it, tio, sigs)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
    assert np.array_equal(got[0][:ntx], ids_l[:ntx])
    assert (got[1] == 1).sum() == len(range(5, ntx, 13))


def test_context_returns_every_byte(small, engine, oracle, ed_vectors, ec_vectors):
    """One smallest-shape call on every path that owns device scratch, in a context of its own
    (64 MiB budget, no idle release): each result against the oracle or the golden expectation,
    cordahip_trim down to what the idle release keeps, and after cordahip_shutdown the GPU's
    account (per GPU, process-wide: the session context reads it) exactly where it was."""
    import json
    import random

    import torch

    import bc_rsa_pss as bc
    import test_cover as TC
    import test_gpu_cover as GC
    import test_gpu_kryo as GK
    import test_gpu_pmt as GP
    import test_gpu_rsa as GR
    import test_gpu_stream as GS
    from conftest import ROOT
    from corda_amd import _lib
    from corda_amd import cover as C
    from corda_amd.corpus import make_c2_corpus, make_c3_corpus
    from corda_amd.engine import Engine
    dev = torch.device("cuda:0")
    rng = random.Random(0xC0DA0701)
    # ---- inputs and references first: the session context must not grow in between ----
    pubs, esig, emsg, _, _ = make_c2_corpus(engine, 128, 0xC0DA0701, dev)
    scheme, ckeys, ckl, csig, csl, cmsg, _, _ = make_c3_corpus(engine, 128, 0xC0DA0702, dev)
    torch.cuda.synchronize()
    k, s, m = (np.ascontiguousarray(x.cpu().numpy()) for x in (pubs, esig, emsg))
    want_ed = np.zeros(128, np.uint8)
    oracle.oracle_ed25519_verify_batch(128, k.ctypes.data, s.ctypes.data, m.ctypes.data, 32, want_ed.ctypes.data, 4)
    sch, K, KL, S, SL, M = (np.ascontiguousarray(x.cpu().numpy()) for x in (scheme, ckeys, ckl, csig, csl, cmsg))
    assert {2, 3} <= set(sch.tolist())  # both curves
    kb = np.ascontiguousarray(np.concatenate([K[i, :KL[i]] for i in range(128)]))
    sb = np.ascontiguousarray(np.concatenate([S[i, :SL[i]] for i in range(128)]))
    ko, so = np.zeros(129, np.uint64), np.zeros(129, np.uint64)
    ko[1:], so[1:] = np.cumsum(KL.astype(np.uint64)), np.cumsum(SL.astype(np.uint64))
    mo = np.arange(129, dtype=np.uint64) * 32
    want_ec = np.zeros(128, np.uint8)
    oracle.oracle_ecdsa_verify_batch(128, sch.ctypes.data, kb.ctypes.data, ko.ctypes.data, sb.ctypes.data,
                                     so.ctypes.data, M.ctypes.data, mo.ctypes.data, want_ec.ctypes.data, 4)
    # RSA-PSS: 64 rows of the 2048-bit class, every fourth signature bit-flipped
    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        rkeys = [dict(x, der=bytes.fromhex(x["der"]), **{n: int(x[n], 16) for n in ("n", "e", "d", "p", "q") if n in x})
                 for x in json.load(f)["keys"]]
    rk = [x for x in GR.signing_keys(rkeys) if GR.class_words(x["n"].bit_length()) == 64][0]
    mod, exp = np.tile(GR.to_words(rk["n"], 64), (64, 1)), np.full(64, rk["e"], np.uint32)
    rsig, rmsg, want_rsa = np.zeros((64, 256), np.uint8), np.zeros((64, 32), np.uint8), []
    for i in range(64):
        msg = rng.randbytes(32)
        sig = GR.fresh_signature(rng, rk, msg, flip=i % 4 == 3)
        rsig[i, :len(sig)] = np.frombuffer(sig, np.uint8)
        rmsg[i] = np.frombuffer(msg, np.uint8)
        want_rsa.append(bc.verify(rk["der"], sig, msg))
    rlen = np.full(64, (rk["n"].bit_length() + 7) // 8, np.uint16)
    assert {bc.OK, bc.BAD_SIG} <= set(want_rsa)
    # coverage: 64 transactions, one or two signer keys each, lists that hold, miss and nest
    cpub = [(ED, rng.randbytes(32)) for _ in range(8)]
    csigs = [[(ED, cpub[(t + j) % 4][1], bytes(64)) for j in range(1 + t % 2)] for t in range(64)]
    trees = [lambda p: [p[0]], lambda p: [p[0], cpub[7]], lambda p: [TC.node(p[0], cpub[7], threshold=1)],
             lambda p: [TC.node(p[0], cpub[6])], lambda p: []]
    must = [trees[t % 5]([(ED, x[1]) for x in csigs[t]]) for t in range(64)]
    cov = C.CoverArrays(*C.flatten_lists(must, None))
    want_cov = C.cover_eval_host(cov, np.zeros(64, np.uint8), csigs)
    assert {0, _lib.TX_SIGNATURES_MISSING} <= set(want_cov[0].tolist())
    # the encoder: 64 items of every kind against the host encoder
    _, kitems = GK._mixed_items(random.Random(77))
    kitems = kitems[:64]
    want_leaves = _lib.kryo_encode(kitems)
    # host signed transactions: 64, ids by the oracle, every seventh transaction's last signature corrupted
    txs = [[bytes([t, q]) * (30 + 20 * q) for q in range(4)] for t in range(64)]
    ids = [GC._oracle_id(oracle, tx) for tx in txs]
    tsigs = []
    for t in range(64):
        per = [(ED,) + _sign(oracle, hashlib.sha256(b"r%d-%d" % (t, q)).digest(), ids[t]) for q in range(1 + t % 3)]
        if t % 7 == 3:
            per[-1] = (ED, per[-1][1], per[-1][2][:9] + bytes([per[-1][2][9] ^ 4]) + per[-1][2][10:])
        tsigs.append(per)
    want_tx = engine.signed_tx_verify(txs, tsigs)
    assert [x.tobytes() for x in want_tx[0]] == ids and (want_tx[1] == 1).sum() == len(range(3, 64, 7))
    (ek, es, em), ecs, want_sed, want_sec = GS._sections(ed_vectors, ec_vectors, 128, 128, 7)
    pmt = GP._cases()
    pmt = [pmt[i % len(pmt)] for i in range(64)]

    def ed_call(e):
        st = torch.full((128,), 0xEE, dtype=torch.uint8, device=dev)
        e.ed25519_verify_device(pubs, esig, emsg, st, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy(), want_ed)

    # ---- 1: the account with only the long-lived contexts, both trimmed (their idle
    # releases then have nothing left to give back while this test runs) ----
    engine.trim()
    small.trim()
    start = engine.device_mem(0)[0]
    old = {n: os.environ.get(n) for n in ("CORDAHIP_DEVICE_MEM_BUDGET", "CORDAHIP_IDLE_RELEASE_MS")}
    os.environ.update(CORDAHIP_DEVICE_MEM_BUDGET="64M", CORDAHIP_IDLE_RELEASE_MS="0")
    try:
        e = Engine(1)
    finally:
        for n, v in old.items():
            if v is None:
                del os.environ[n]
            else:
                os.environ[n] = v
    try:
        post_init = e.device_mem(0)[0]
        assert post_init > start and e.device_mem(0)[2] == 64 * MIB
        # ---- 3: every path that owns scratch ----
        ed_call(e)
        st = torch.full((128,), 0xEE, dtype=torch.uint8, device=dev)
        e.ecdsa_verify_device(scheme, ckeys, ckl, csig, csl, cmsg, st, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert np.array_equal(st.cpu().numpy(), want_ec)
        up = lambda a, ty: torch.from_numpy(a.view(ty).copy()).to(dev)  # noqa: E731
        st = torch.full((64,), 0xEE, dtype=torch.uint8, device=dev)
        e.rsa_pss_verify_device(up(mod, np.int32), up(exp, np.int32), up(rsig, np.uint8), up(rlen, np.int16),
                                up(rmsg, np.uint8), st, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert st.cpu().numpy().tolist() == want_rsa
        cs, ct = cov.to_device()
        so_, _, kb_, _ = C.sig_key_arrays(csigs)
        tst = torch.zeros(64, dtype=torch.uint8, device=dev)
        e.tx_cover_device(64, tst, torch.tensor(so_.astype(np.int64), device=dev),
                          torch.tensor(np.concatenate([kb_, np.zeros(32, np.uint8)]), device=dev), cs)
        torch.cuda.synchronize()
        req, first = cov.from_device(ct)
        assert np.array_equal(tst.cpu().numpy(), want_cov[0]) and np.array_equal(req, want_cov[1])
        assert np.array_equal(first, want_cov[2])
        out, off, status = e.kryo_encode_packed_device(*_lib.kryo_pack(kitems))
        assert int(status.sum()) == 0 and GK._leaves(out, off, 64) == want_leaves
        got = e.signed_tx_verify(txs, tsigs)
        assert all(np.array_equal(a, b) for a, b in zip(got, want_tx))
        sed, sec = np.zeros(128, np.uint8), np.zeros(128, np.uint8)
        e.stream_verify((ek, es, em, sed), ecs + (sec,))
        assert sed.tolist() == want_sed and sec.tolist() == want_sec
        assert [int(x) for x in e.filtered_tx_verify([c[0] for c in pmt])] == [c[1] for c in pmt]
        # ---- 4: trim leaves the fixed tables, the encoder's table and the counters ----
        grown = e.device_mem(0)[0]
        e.trim()
        trimmed = e.device_mem(0)[0]
        e.trim()
        assert e.device_mem(0)[0] == trimmed
        # (the encoder's table is 90.9 MiB whatever the budget; the counters 64 bytes per ECDSA slot in use)
        assert post_init < trimmed < grown and trimmed - post_init < 96 * MIB
        # ---- 5: and the context still verifies ----
        ed_call(e)
    finally:
        e.close()
    # ---- 6: every byte is back ----
    assert engine.device_mem(0)[0] == start
