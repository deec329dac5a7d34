"""The notary commit log on the GPU (K16: cordahip_commit_log_*, cordahip_commit_inputs and its
ticketed and device-resident forms) against the serial model tests/commit_log_model.py: every
tx_status, committed byte, ref_state and ref_by row of every batch, and after each batch the
lookup of the whole ref universe against the model's dict. Tiny shapes; the batches are dense
in collisions (40 refs, 8 transaction ids, 3 callers) so that retries, cross-caller conflicts
and in-batch dependencies all occur."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import commit_log_worker as W
from commit_log_model import (COMMIT_CONFLICT, COMMIT_SKIPPED, COMMIT_TIME_WINDOW_INVALID, OK, REF_ABSENT, REF_OTHER,
                              REF_SELF, CommitLogModel)
from corda_amd import _lib
from corda_amd._lib import EngineError, lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
h, ref = W.h, W.ref
ALICE, BOB = 7, 8


@pytest.fixture
def log(engine):
    lid = engine.commit_log_create(10, salt=bytes(range(16)))
    yield lid
    engine.commit_log_destroy(lid)


def check(engine, lid, model, txs, universe, **kw):
    """One batch through the GPU and the model: all four outputs, then the universe's lookup."""
    st, cm, rs, rb = engine.commit_inputs(lid, txs, **kw)
    want = model.commit_batch(txs, **kw)
    assert ([int(x) for x in st], [int(x) for x in cm], rs, rb) == tuple(want)
    look = engine.commit_log_lookup(lid, universe)
    assert look == [model.log.get((bytes(r[0]), r[1])) for r in universe]
    assert engine.commit_log_stats(lid)[0] == len(model.log)
    return want


# ---- 1. parity, dense collisions ------------------------------------------------------------
@pytest.mark.parametrize("ntx", W.NTX)
def test_dense_batches_equal_the_model(engine, ntx):
    want = W.model_dense(ntx)
    assert W.run_dense(engine, ntx) == want
    if ntx >= 63:  # the batches are what they are meant to be: every outcome occurs
        sts = [s for b in want for s in b[0][0]]
        cms = [c for b in want for c in b[0][1]]
        assert sts.count(COMMIT_CONFLICT) > 10 and cms.count(1) > 5
        assert sum(1 for s, c in zip(sts, cms) if s == OK and c == 0) > 0


@pytest.mark.parametrize("rounds", ["0", "1"])
def test_round_count_changes_nothing(rounds):
    """CORDAHIP_COMMIT_ROUNDS=0 (the in-order sweep alone) and =1 in processes of their own."""
    env = dict(os.environ, CORDAHIP_COMMIT_ROUNDS=rounds)
    p = subprocess.run([sys.executable, os.path.join(HERE, "commit_log_worker.py")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    for ntx in W.NTX:
        assert got[str(ntx)] == W.model_dense(ntx), ntx


# ---- 2. chain ---------------------------------------------------------------------------------
def test_chain_is_decided_in_order(engine, log):
    """t_k = {r_k, r_k+1}: the even transactions commit and each odd one conflicts on exactly
    one ref -- r_k, stored by t_k-1 at position 1; r_k+1 is still absent when t_k is reached.
    The chain is longer than any round count, so the in-order sweep decides it."""
    n = 41
    txs = [(h("chain", k), ALICE, [ref(k), ref(k + 1)], None) for k in range(n)]
    m = CommitLogModel()
    st, cm, rs, rb = check(engine, log, m, txs, [ref(i) for i in range(n + 1)])
    assert st == [OK if k % 2 == 0 else COMMIT_CONFLICT for k in range(n)]
    assert cm == [1 - k % 2 for k in range(n)]
    for k in range(1, n, 2):
        assert rs[k] == [REF_OTHER, REF_ABSENT] and rb[k] == [(h("chain", k - 1), 1, ALICE), None]


# ---- 3. the four quirks by name -----------------------------------------------------------------
def test_retry_in_batch_and_across_batches(engine, log):
    m, uni = CommitLogModel(), [ref(i) for i in range(4)]
    req = (h("tx", 1), ALICE, [ref(0), ref(1)], None)
    st, cm, rs, _ = check(engine, log, m, [req, req], uni)
    assert st == [OK, OK] and cm == [1, 0] and rs[1] == [REF_SELF, REF_SELF]
    st, cm, _, _ = check(engine, log, m, [req], uni)
    assert st == [OK] and cm == [0]


def test_same_id_from_another_caller_conflicts(engine, log):
    m, uni = CommitLogModel(), [ref(i) for i in range(4)]
    check(engine, log, m, [(h("tx", 1), ALICE, [ref(0)], None)], uni)
    st, cm, rs, rb = check(engine, log, m, [(h("tx", 1), BOB, [ref(0)], None)], uni)
    assert (st, cm, rs, rb) == ([COMMIT_CONFLICT], [0], [[REF_OTHER]], [[(h("tx", 1), 0, ALICE)]])


def test_duplicated_ref_commits_then_conflicts_with_itself(engine, log):
    m, uni = CommitLogModel(), [ref(i) for i in range(4)]
    req = (h("tx", 1), ALICE, [ref(0), ref(1), ref(0)], None)
    st, cm, _, _ = check(engine, log, m, [req], uni)
    assert (st, cm) == ([OK], [1])
    assert engine.commit_log_lookup(log, [ref(0)]) == [(h("tx", 1), 2, ALICE)]  # the last position
    assert engine.commit_log_stats(log)[0] == 2
    st, cm, rs, rb = check(engine, log, m, [req], uni)
    assert (st, cm, rs) == ([COMMIT_CONFLICT], [0], [[REF_OTHER, REF_SELF, REF_SELF]])
    assert rb[0][0] == (h("tx", 1), 2, ALICE)
    # ... and in one batch too
    req2 = (h("tx", 2), BOB, [ref(2), ref(2)], None)
    st, cm, rs, _ = check(engine, log, m, [req2, req2], uni)
    assert st == [OK, COMMIT_CONFLICT] and cm == [1, 0] and rs[1] == [REF_OTHER, REF_SELF]


def test_already_committed_inserts_no_absent_input(engine, log):
    m, uni = CommitLogModel(), [ref(i) for i in range(4)]
    check(engine, log, m, [(h("tx", 1), ALICE, [ref(0)], None)], uni)
    st, cm, rs, _ = check(engine, log, m, [(h("tx", 1), ALICE, [ref(0), ref(1)], None)], uni)
    assert (st, cm, rs) == ([OK], [0], [[REF_SELF, REF_ABSENT]])
    assert engine.commit_log_lookup(log, [ref(1)]) == [None]
    # a conflicting transaction leaves its other inputs for a later one of the same batch
    txs = [(h("tx", 2), ALICE, [ref(0), ref(2)], None), (h("tx", 3), BOB, [ref(2)], None)]
    st, cm, _, _ = check(engine, log, m, txs, uni)
    assert st == [COMMIT_CONFLICT, OK] and cm == [0, 1]


# ---- 4. table edges -------------------------------------------------------------------------------
def test_small_table_to_seven_eighths_then_full_then_reserve(engine):
    lid = engine.commit_log_create(6, salt=b"edge-of-the-tab!")
    try:
        m = CommitLogModel()
        uni = [ref(1000 + i) for i in range(60)]
        txs = [(h("fill", t), ALICE, uni[4 * t:4 * t + 4], None) for t in range(14)]
        check(engine, lid, m, txs, uni)  # 56 entries in 64 slots: probe sequences wrap the table's end
        assert engine.commit_log_stats(lid) == (56, 64, 15)
        assert all(b is not None for b in engine.commit_log_lookup(lid, uni[:56]))
        # the next call would pass 7/8: refused before any enqueue, outputs and log untouched
        n1 = np.full(1, 0xA5, np.uint8)
        st, cmm, rs = n1.copy(), n1.copy(), n1.copy()
        rb = np.full(40, 0xA5, np.uint8)
        txid = np.frombuffer(h("late"), np.uint8).copy()
        caller = np.array([ALICE], np.uint32)
        refs = engine._state_refs([uni[56]])
        off = np.array([0, 1], np.uint64)
        b = _lib.CommitBatch(1, txid.ctypes.data, caller.ctypes.data, refs.ctypes.data, off.ctypes.data, 1, None, None,
                             0, 0, None, st.ctypes.data, cmm.ctypes.data, rs.ctypes.data, rb.ctypes.data)
        assert lib().cordahip_commit_inputs(engine.ctx, lid, ctypes.byref(b)) == _lib.ERR_LOG_FULL
        assert st[0] == cmm[0] == rs[0] == 0xA5 and (rb == 0xA5).all()
        assert engine.commit_log_stats(lid) == (56, 64, 15)
        assert engine.commit_log_lookup(lid, uni) == [m.log.get(r) for r in uni]
        with pytest.raises(EngineError) as e:
            engine.commit_log_load(lid, [(uni[57], (h("x"), 0, 1))])
        assert e.value.code == _lib.ERR_LOG_FULL
        # a call with no inputs adds nothing and still passes
        assert [int(x) for x in engine.commit_inputs(lid, [(h("empty"), ALICE, [], None)])[0]] == [OK]
        m.commit_batch([(h("empty"), ALICE, [], None)])
        # reserve: every entry survives the rehash, and there is room again
        engine.commit_log_reserve(lid, 8)
        assert engine.commit_log_stats(lid)[:2] == (56, 256)
        assert engine.commit_log_lookup(lid, uni) == [m.log.get(r) for r in uni]
        engine.commit_log_reserve(lid, 7)  # never shrinks
        assert engine.commit_log_stats(lid)[1] == 256
        st, cm, _, _ = check(engine, lid, m, [(h("late"), ALICE, [uni[56], uni[0]], None),
                                              (h("late"), ALICE, [uni[56]], None)], uni)
        assert st == [COMMIT_CONFLICT, OK] and cm == [0, 1]
    finally:
        engine.commit_log_destroy(lid)


# ---- 5. gate, time window, load, ids, arguments ------------------------------------------------------
def test_gate_and_time_window(engine, log):
    m, uni = CommitLogModel(), [ref(i) for i in range(8)]
    now, tol = 1_500_000_000_000_000_000, 30_000_000_000
    wins = [None, (None, now - tol), (None, now - tol - 1), (now + tol, None), (now + tol + 1, None),
            (now - 5, now + 5), (-(1 << 70), 1 << 70), (1 << 70, None)]
    txs = [(h("tw", t), ALICE, [ref(t)], w) for t, w in enumerate(wins)]
    st, cm, _, _ = check(engine, log, m, txs, uni, now_ns=now, tolerance_ns=tol, gate=[0, 0, 0, 0, 0, 9, 0, 0])
    T = COMMIT_TIME_WINDOW_INVALID
    assert st == [OK, OK, T, OK, T, COMMIT_SKIPPED, OK, T] and cm == [1, 1, 0, 1, 0, 0, 1, 0]
    # nothing was looked up or inserted for the skipped and the out-of-window ones
    assert engine.commit_log_lookup(log, [ref(2), ref(4), ref(5), ref(7)]) == [None] * 4
    for bad in (dict(now_ns=1 << 61), dict(now_ns=-(1 << 61)), dict(tolerance_ns=-1), dict(tolerance_ns=1 << 61)):
        with pytest.raises(EngineError) as e:
            engine.commit_inputs(log, txs[:1], **bad)
        assert e.value.code == _lib.ERR_INVALID_ARG


def test_load_then_commit(engine, log):
    m = CommitLogModel()
    uni = [ref(i) for i in range(12)]
    rows = [(ref(i), (h("old", i), i % 3, 1 + i % 2)) for i in range(8)]
    assert engine.commit_log_load(log, rows) == m.load(rows) == 0
    again = rows[2:5] + [(ref(9), (h("old", 9), 0, 1)), (ref(9), (h("other", 9), 1, 2))]
    assert engine.commit_log_load(log, again) == m.load(again) == 4  # three old ones, one twice in the call
    assert engine.commit_log_stats(log) == (9, 1024, 1)
    assert engine.commit_log_lookup(log, uni) == [m.log.get(r) for r in uni]
    txs = [(h("old", 0), 1, [ref(0)], None),            # the loaded record itself: already committed
           (h("new", 1), 1, [ref(1), ref(10)], None),   # a loaded ref: conflict
           (h("new", 2), 1, [ref(10), ref(11)], None)]
    st, cm, _, _ = check(engine, log, m, txs, uni)
    assert st == [OK, COMMIT_CONFLICT, OK] and cm == [0, 0, 1]


def test_ids_and_arguments(engine):
    a = engine.commit_log_create(6)
    b = engine.commit_log_create(6)
    assert a != b and a != 0 and b != 0
    engine.commit_log_destroy(a)
    c = engine.commit_log_create(6)
    assert c not in (a, b)  # an id is never reused
    for call in (lambda: engine.commit_log_destroy(a), lambda: engine.commit_log_stats(a),
                 lambda: engine.commit_log_reserve(a, 8), lambda: engine.commit_log_lookup(a, [ref(0)]),
                 lambda: engine.commit_log_load(a, [(ref(0), (h("x"), 0, 1))]),
                 lambda: engine.commit_inputs(a, [(h("x"), 1, [ref(0)], None)]),
                 lambda: engine.commit_log_create(5), lambda: engine.commit_log_create(33),
                 lambda: engine.commit_log_create(6, device=9)):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.code == _lib.ERR_INVALID_ARG
    # offsets that decrease, or run past n_refs: refused whole
    txid = np.frombuffer(h("a") + h("b"), np.uint8).copy()
    caller = np.array([1, 1], np.uint32)
    refs = engine._state_refs([ref(0), ref(1)])
    st, cm, rs = np.zeros(2, np.uint8), np.zeros(2, np.uint8), np.zeros(2, np.uint8)
    rb = np.zeros(80, np.uint8)
    for off, n_refs in (([0, 2, 1], 2), ([0, 1, 3], 2), ([1, 1, 2], 1)):
        o = np.array(off, np.uint64)
        bt = _lib.CommitBatch(2, txid.ctypes.data, caller.ctypes.data, refs.ctypes.data, o.ctypes.data, n_refs, None,
                              None, 0, 0, None, st.ctypes.data, cm.ctypes.data, rs.ctypes.data, rb.ctypes.data)
        assert lib().cordahip_commit_inputs(engine.ctx, b, ctypes.byref(bt)) == _lib.ERR_INVALID_ARG
    assert engine.commit_log_stats(b) == (0, 64, 1)
    engine.commit_log_destroy(b)
    engine.commit_log_destroy(c)


def test_tickets_commit_in_submit_order(engine, log):
    m, uni = CommitLogModel(), [ref(i) for i in range(40)]
    batches = W.dense_batches(17, seed=7)
    tickets = [engine.commit_inputs_submit(log, txs) for txs in batches]
    for txs, t in zip(batches, tickets):
        st, cm, rs, rb = t.wait()
        assert ([int(x) for x in st], [int(x) for x in cm], rs, rb) == tuple(m.commit_batch(txs))
    assert engine.commit_log_lookup(log, uni) == [m.log.get(r) for r in uni]


def test_memory_is_accounted_and_kept_by_trim(engine):
    def in_use():
        u = ctypes.c_uint64()
        assert lib().cordahip_device_mem(engine.ctx, 0, ctypes.byref(u), None, None) == 0
        return u.value
    before = in_use()
    lid = engine.commit_log_create(12)
    table = 96 << 12
    assert in_use() - before >= table
    engine.commit_inputs(lid, [(h("tx", 1), ALICE, [ref(0)], None)])
    assert lib().cordahip_trim(engine.ctx) == 0
    assert in_use() - before >= table  # the log survives cordahip_trim ...
    assert engine.commit_log_lookup(lid, [ref(0)]) == [(h("tx", 1), 0, ALICE)]  # ... with its entries
    engine.commit_log_destroy(lid)
    assert lib().cordahip_trim(engine.ctx) == 0
    assert in_use() <= before


# ---- 6. the device-resident chain: verify -> commit -> sign on one stream ------------------------------
def test_device_chain_gates_the_signer(engine, oracle):
    import hashlib

    import torch
    dev = torch.device("cuda:0")
    seed = hashlib.sha256(b"notary-key").digest()
    kid, pub = engine.signer_add_ed25519(seed)
    lid = engine.commit_log_create(10)
    try:
        m = CommitLogModel()
        now, tol = 10**18, 10**9
        txs = [(h("dtx", 0), ALICE, [ref(0), ref(1)], None),
               (h("dtx", 1), BOB, [ref(1)], None),                    # conflict with the one before it
               (h("dtx", 2), BOB, [ref(2)], (None, now - tol - 1)),   # out of window
               (h("dtx", 3), BOB, [ref(3)], None),                    # gated by the earlier stage
               (h("dtx", 0), ALICE, [ref(0), ref(1)], None),          # retry: signed again
               (h("dtx", 5), BOB, [], None)]
        gate = [0, 0, 0, 2, 0, 0]
        want = m.commit_batch(txs, now_ns=now, tolerance_ns=tol, gate=gate)
        n = len(txs)
        flat = [r for tx in txs for r in tx[2]]
        nr = len(flat)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(tx[2]) for tx in txs])
        absent = _lib.TW_SIDE_ABSENT
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_txid = to(np.frombuffer(b"".join(tx[0] for tx in txs), np.uint8).reshape(n, 32).copy())
        d_caller = to(np.array([tx[1] for tx in txs], np.int32))
        d_refs = to(engine._state_refs(flat).view(np.uint8).reshape(-1, 36)[:nr].copy())
        d_off = to(off)
        d_from = to(np.array([absent if not tx[3] or tx[3][0] is None else tx[3][0] for tx in txs], np.int64))
        d_until = to(np.array([absent if not tx[3] or tx[3][1] is None else tx[3][1] for tx in txs], np.int64))
        d_gate = to(np.array(gate, np.uint8))
        d_st = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        d_cm = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        d_rs = torch.full((nr,), 0xA5, dtype=torch.uint8, device=dev)
        d_rb = torch.full((nr, 40), 0xA5, dtype=torch.uint8, device=dev)
        d_kid = to(np.full(n, kid, np.int64).astype(np.uint32).view(np.int32))
        d_sig = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
        d_sst = torch.zeros(n, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            engine.commit_inputs_device(lid, d_txid, d_caller, d_refs, d_off, d_st, d_cm, d_rs, d_rb, tw_from=d_from,
                                        tw_until=d_until, now_ns=now, tolerance_ns=tol, gate=d_gate, stream=stream)
            engine.ed25519_sign_keyed_device(d_kid, d_txid, d_sig, d_sst, gate=d_st, stream=stream)
        stream.synchronize()
        st, cm = d_st.cpu().numpy(), d_cm.cpu().numpy()
        assert [int(x) for x in st] == want[0] and [int(x) for x in cm] == want[1]
        assert want[0] == [OK, COMMIT_CONFLICT, COMMIT_TIME_WINDOW_INVALID, COMMIT_SKIPPED, OK, OK]
        rs, rb = d_rs.cpu().numpy(), d_rb.cpu().numpy()
        assert [int(x) for x in rs] == [s for row in want[2] for s in row]
        for i, by in enumerate(b for row in want[3] for b in row):
            row = rb[i].tobytes()
            assert row == (bytes(40) if by is None else
                           by[0] + by[1].to_bytes(4, "little") + by[2].to_bytes(4, "little")), i
        sst, sig = d_sst.cpu().numpy(), d_sig.cpu().numpy()
        sig_buf, pub_buf = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)
        for t, tx in enumerate(txs):
            if want[0][t] == OK:
                oracle.oracle_ed25519_sign(seed, tx[0], 32, pub_buf, sig_buf)
                assert sst[t] == OK and sig[t].tobytes() == sig_buf.raw and pub_buf.raw == pub, t
            else:
                assert sst[t] == _lib.SIGN_SKIPPED and not sig[t].any(), t
        uni = [ref(i) for i in range(6)]
        assert engine.commit_log_lookup(lid, uni) == [m.log.get(r) for r in uni]
    finally:
        engine.commit_log_destroy(lid)
        engine.signer_remove(kid)


def test_notarise_filtered_transactions(engine, oracle):
    """resolve.notarise_filtered_transactions: verify -> commit -> sign, the NotaryErrors and the
    rows to persist, against the model and the signing oracle."""
    import hashlib

    from corda_amd import resolve as R
    cases = json.load(open(os.path.join(HERE, "golden", "pmt_vectors.json")))["cases"]
    by_root = {}
    for c in cases:  # five verifying tear-offs with distinct ids
        if c["status"] == 0:
            by_root.setdefault(c["root"], ([bytes.fromhex(x) for x in c["leaves"]],
                                           [(t, bytes.fromhex(hh) if hh else None) for t, hh in c["tokens"]],
                                           bytes.fromhex(c["root"])))
    ftxs = list(by_root.values())[:5]
    assert len(ftxs) == 5 and len({f[2] for f in ftxs}) == 5
    leaves, toks, root = ftxs[3]
    ftxs[3] = (leaves, toks, bytes([root[0] ^ 1]) + root[1:])  # a tear-off that does not verify
    ftxs.append(ftxs[0])                                        # the first request again: signed again
    now, tol = 10**18, 10**9
    inputs = [[ref(0), ref(1)], [ref(1), ref(2)], [ref(3)], [ref(4)], [ref(5), ref(5)], [ref(0), ref(1)]]
    windows = [None, None, (now + tol + 1, None), None, None, None]
    callers = [ALICE, BOB, BOB, BOB, BOB, ALICE]
    seed = hashlib.sha256(b"notary-key-2").digest()
    kid, _ = engine.signer_add_ed25519(seed)
    lid = engine.commit_log_create(8)
    try:
        answers, rows = R.notarise_filtered_transactions(engine, lid, ftxs, inputs, windows, callers, kid, now, tol)
        sig_buf, pub_buf = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)

        def signed(t):
            oracle.oracle_ed25519_sign(seed, ftxs[t][2], 32, pub_buf, sig_buf)
            return sig_buf.raw
        assert answers[0] == signed(0) and answers[5] == signed(5) == signed(0) and answers[4] == signed(4)
        assert answers[1] == R.NotaryError("Conflict", ftxs[1][2], {ref(1): (ftxs[0][2], 1, ALICE)})
        assert answers[2] == R.NotaryError("TimeWindowInvalid", ftxs[2][2])
        assert answers[3] == R.NotaryError("TransactionInvalid", ftxs[3][2])
        assert rows == [(ref(0), (ftxs[0][2], 0, ALICE)), (ref(1), (ftxs[0][2], 1, ALICE)),
                        (ref(5), (ftxs[4][2], 1, BOB))]
        uni = [ref(i) for i in range(6)]
        assert engine.commit_log_lookup(lid, uni) == [dict(rows).get(r) for r in uni]
        assert R.notarise_filtered_transactions(engine, lid, [], [], [], [], kid, now, tol) == ([], [])
    finally:
        engine.commit_log_destroy(lid)
        engine.signer_remove(kid)
