"""The serial model of the notary's uniqueness check (tests/commit_log_model.py) against the
reference's two structural cases (PersistentUniquenessProviderTests.kt:35-59) and the
consequences the commit log's contract pins, and corda_amd.resolve.commit_input_states (the
product's pure-Python mirror) against the model on seeded random batches. CPU only."""
import hashlib
import random

import pytest

from commit_log_model import (COMMIT_CONFLICT, COMMIT_SKIPPED, COMMIT_TIME_WINDOW_INVALID, OK, REF_ABSENT, REF_OTHER,
                              REF_SELF, CommitLogModel, window_valid)


def h(tag, i=0):
    return hashlib.sha256(b"%s-%d" % (tag.encode(), i)).digest()


def ref(i, index=0):
    return (h("state", i), index)


TX, TX2 = h("tx", 1), h("tx", 2)
ALICE, BOB = 7, 8


def test_commits_a_transaction_with_unused_inputs():
    """`should commit a transaction with unused inputs without exception` (:35-42)"""
    m = CommitLogModel()
    assert m.commit_batch([(TX, ALICE, [ref(0)], None)]) == ([OK], [1], [[REF_ABSENT]], [[None]])
    assert m.log == {ref(0): (TX, 0, ALICE)}


def test_reports_previously_used_inputs():
    """`should report a conflict for a transaction with previously used inputs` (:44-59): the
    provider's stateHistory names the consuming id, the input's index and the requesting party.
    (The provider throws for the retry too; the service above it swallows that one.)"""
    m = CommitLogModel()
    m.commit_batch([(TX, ALICE, [ref(0)], None)])
    st, cm, rs, rb = m.commit_batch([(TX2, ALICE, [ref(0)], None)])
    assert (st, cm, rs) == ([COMMIT_CONFLICT], [0], [[REF_OTHER]])
    assert rb == [[(TX, 0, ALICE)]]


def test_same_request_twice_is_ok_in_one_batch_and_across():
    m = CommitLogModel()
    req = (TX, ALICE, [ref(0), ref(1)], None)
    st, cm, rs, rb = m.commit_batch([req, req])
    assert st == [OK, OK] and cm == [1, 0]
    assert rs[1] == [REF_SELF, REF_SELF] and rb[1] == [(TX, 0, ALICE), (TX, 1, ALICE)]
    st, cm, _, _ = m.commit_batch([req])
    assert st == [OK] and cm == [0]


def test_same_txid_from_another_caller_conflicts():
    m = CommitLogModel()
    m.commit_batch([(TX, ALICE, [ref(0)], None)])
    st, cm, rs, rb = m.commit_batch([(TX, BOB, [ref(0)], None)])
    assert (st, cm, rs, rb) == ([COMMIT_CONFLICT], [0], [[REF_OTHER]], [[(TX, 0, ALICE)]])


def test_duplicated_ref_commits_then_conflicts_with_itself():
    m = CommitLogModel()
    req = (TX, ALICE, [ref(0), ref(1), ref(0)], None)
    assert m.commit_batch([req])[:2] == ([OK], [1])
    assert m.log[ref(0)] == (TX, 2, ALICE)  # the last put wins
    st, cm, rs, rb = m.commit_batch([req])
    assert (st, cm) == ([COMMIT_CONFLICT], [0])
    assert rs == [[REF_OTHER, REF_SELF, REF_SELF]]  # position 0 no longer equals the stored index
    assert rb == [[(TX, 2, ALICE), (TX, 1, ALICE), (TX, 2, ALICE)]]


def test_conflicting_transaction_consumes_nothing():
    m = CommitLogModel()
    m.commit_batch([(TX, ALICE, [ref(0)], None)])
    st, cm, rs, _ = m.commit_batch([(TX2, ALICE, [ref(0), ref(1)], None), (h("tx", 3), BOB, [ref(1)], None)])
    assert st == [COMMIT_CONFLICT, OK] and cm == [0, 1] and rs[0] == [REF_OTHER, REF_ABSENT]
    assert m.log[ref(1)] == (h("tx", 3), 0, BOB)


def test_already_committed_inserts_nothing():
    m = CommitLogModel()
    m.commit_batch([(TX, ALICE, [ref(0)], None)])
    # the same id and caller, input 0 the same, a second input the log has not seen
    st, cm, rs, _ = m.commit_batch([(TX, ALICE, [ref(0), ref(1)], None)])
    assert (st, cm, rs) == ([OK], [0], [[REF_SELF, REF_ABSENT]])
    assert ref(1) not in m.log


def test_no_inputs_commits_and_gate_and_window_touch_nothing():
    m = CommitLogModel()
    st, cm, rs, rb = m.commit_batch([(TX, ALICE, [], None), (TX2, ALICE, [ref(0)], None),
                                     (TX2, ALICE, [ref(1)], (None, 89))], now_ns=100, tolerance_ns=10, gate=[0, 3, 0])
    assert st == [OK, COMMIT_SKIPPED, COMMIT_TIME_WINDOW_INVALID] and cm == [1, 0, 0]
    assert rs == [[], [REF_ABSENT], [REF_ABSENT]] and rb == [[], [None], [None]] and m.log == {}


def test_window_is_exact_in_nanoseconds():
    now, tol = 1_500_000_000_000_000_000, 30_000_000_000
    assert window_valid((None, now - tol), now, tol) and not window_valid((None, now - tol - 1), now, tol)
    assert window_valid((now + tol, None), now, tol) and not window_valid((now + tol + 1, None), now, tol)
    assert window_valid((None, None), now, tol) and window_valid(None, now, tol)
    assert window_valid((now - 5, now + 5), now, 0) and not window_valid((now + 1, now + 5), now, 0)
    # saturated sides
    assert window_valid((-(1 << 62), 1 << 62), now, tol) and not window_valid((1 << 62, None), now, tol)


def random_batch(rng, ntx):
    txs, gate = [], []
    for _ in range(ntx):
        refs = [ref(rng.randrange(40), rng.randrange(2)) for _ in range(rng.randrange(6))]
        win = None
        if rng.random() < 0.4:
            win = (rng.choice([None, 90, 111, 110]), rng.choice([None, 110, 89, 90]))
        txs.append((h("tx", rng.randrange(8)), rng.randrange(3), refs, win))
        gate.append(1 if rng.random() < 0.1 else 0)
    return txs, gate


@pytest.mark.parametrize("seed", range(8))
def test_resolve_commit_input_states_equals_the_model(seed):
    from corda_amd import resolve
    rng = random.Random(20261020 + seed)
    m, log = CommitLogModel(), {}
    rows = [(ref(100 + i), (h("old", i), i, 1)) for i in range(5)]
    assert m.load(rows + rows[:2]) == 2
    log.update((r, by) for r, by in rows)
    seen = set()
    for _ in range(6):
        txs, gate = random_batch(rng, rng.choice([0, 1, 2, 17, 64]))
        g = gate if rng.random() < 0.5 else None
        want = m.commit_batch(txs, now_ns=100, tolerance_ns=10, gate=g)
        got = resolve.commit_input_states(log, txs, now_ns=100, tolerance_ns=10, gate=g)
        assert got == want
        assert log == m.log
        seen.update(want[0])
    assert seen >= {OK, COMMIT_CONFLICT, COMMIT_TIME_WINDOW_INVALID}
