"""tests/commit_revoke_model.py's own properties (CPU-only): revoke and export as the header
states them, the sequence numbers, and the slot-level simulation's invariants."""
import hashlib
import random

from commit_log_model import COMMIT_CONFLICT, OK, CommitLogModel
from commit_revoke_model import RevokeModel, TableSim

ALICE, BOB = 7, 8


def h(tag, i=0):
    return hashlib.sha256(b"%s-%d" % (tag.encode(), i)).digest()


def ref(i):
    return (h("state", i // 2), i % 2)


def test_revoke_then_recommit():
    m = RevokeModel()
    req = (h("tx", 1), ALICE, [ref(0), ref(1)], None)
    assert m.commit_batch([req])[:2] == ([OK], [1])
    assert m.commit_batch([req])[:2] == ([OK], [0])  # the retry: nothing to persist
    rows = [(ref(0), (h("tx", 1), 0, ALICE)), (ref(1), (h("tx", 1), 1, ALICE))]
    assert m.revoke(rows) == ([1, 1], 2) and m.log == {} and m.seq == {}
    assert m.commit_batch([req])[:2] == ([OK], [1])  # now there is: committed again
    assert m.revoke(rows) == ([1, 1], 2)
    assert m.commit_batch([(h("tx", 2), BOB, [ref(1)], None)])[:2] == ([OK], [1])  # another spender commits
    assert m.next_seq == 5  # revokes consume no sequence number


def test_revoke_of_another_id_index_or_caller_is_a_no_op():
    m = RevokeModel()
    m.commit_batch([(h("tx", 1), ALICE, [ref(0), ref(1)], None)])
    before = dict(m.log)
    rows = [(ref(0), (h("tx", 2), 0, ALICE)), (ref(0), (h("tx", 1), 1, ALICE)), (ref(0), (h("tx", 1), 0, BOB)),
            (ref(5), (h("tx", 1), 0, ALICE))]
    assert m.revoke(rows) == ([0, 0, 0, 0], 0) and m.log == before
    assert m.commit_batch([(h("tx", 3), BOB, [ref(0)], None)])[0] == [COMMIT_CONFLICT]


def test_duplicate_rows_count_once_and_a_doubled_ref_goes_by_its_last_position():
    m = RevokeModel()
    m.commit_batch([(h("tx", 1), ALICE, [ref(0), ref(1), ref(0)], None)])
    first, last = (ref(0), (h("tx", 1), 0, ALICE)), (ref(0), (h("tx", 1), 2, ALICE))
    assert m.revoke([first]) == ([0], 0)
    assert m.revoke([last, first, last, last]) == ([1, 0, 1, 1], 1)
    assert list(m.log) == [ref(1)]


def test_sequence_numbers_and_export():
    m = RevokeModel()
    assert m.export() == []
    m.load([(ref(10), (h("old", 0), 0, BOB)), (ref(10), (h("old", 1), 0, BOB))])
    txs = [(h("tx", 1), ALICE, [ref(0)], None), (h("tx", 2), ALICE, [ref(0)], None), (h("tx", 3), BOB, [ref(1)], None)]
    m.commit_batch(txs, gate=[0, 0, 0])
    base = m.next_seq
    assert base == 4
    m.commit_batch([(h("tx", 4), ALICE, [], None), (h("tx", 5), ALICE, [ref(2), ref(3)], None)])
    assert sorted(m.export()) == sorted([(ref(10), (h("old", 0), 0, BOB), 0), (ref(0), (h("tx", 1), 0, ALICE), 1),
                                         (ref(1), (h("tx", 3), 0, BOB), 3), (ref(2), (h("tx", 5), 0, ALICE), 5),
                                         (ref(3), (h("tx", 5), 1, ALICE), 5)])
    assert sorted(r for r, _, _ in m.export(base)) == sorted([ref(2), ref(3)])
    m.revoke([(ref(2), (h("tx", 5), 0, ALICE))])
    assert [r for r, _, _ in m.export(base)] == [ref(3)]


def test_the_base_model_is_unchanged_underneath():
    rng = random.Random(5)
    a, b = CommitLogModel(), RevokeModel()
    for _ in range(20):
        txs = [(h("tx", rng.randrange(8)), rng.randrange(3), [ref(rng.randrange(20)) for _ in range(rng.randrange(4))],
                None) for _ in range(9)]
        gate = [rng.randrange(4) == 0 for _ in txs]
        assert tuple(a.commit_batch(txs, gate=gate)) == tuple(b.commit_batch(txs, gate=gate))
    assert a.log == b.log and set(b.seq) == set(b.log)


def test_table_simulation_keeps_every_key_reachable():
    """Random puts and erases at 7/8 load in 64 slots: every live key found, every erased key gone,
    and the occupied slots those of a table into which the erased keys were never put."""
    rng = random.Random(11)
    salt = bytes(range(16))
    for _ in range(50):
        sim, live = TableSim(6, salt), []
        pool = [ref(rng.randrange(10 ** 6)) for _ in range(56)]
        for r in pool:
            sim.put(r)
            live.append(r)
        rng.shuffle(live)
        gone = [live.pop() for _ in range(rng.randrange(1, 40))]
        for r in gone:
            sim.erase(r)
        assert all(sim.slot_of(r) is not None for r in live) and all(sim.slot_of(r) is None for r in gone)
        fresh = TableSim(6, salt)
        for r in pool:
            if r in live:
                fresh.put(r)
        assert [s is None for s in sim.slots] == [s is None for s in fresh.slots]
        assert sum(len(c) for c in sim.clusters()) == sim.entries() == len(set(live))
