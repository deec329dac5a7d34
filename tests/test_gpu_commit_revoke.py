"""cordahip_commit_log_revoke and cordahip_commit_log_export on the GPU against
tests/commit_revoke_model.py: after every step the call's outputs, then the lookup of the whole
universe, then cordahip_commit_log_stats's entry count. The cluster cases run on a 64-slot log
whose layout tests/commit_revoke_worker.py builds entry by entry and the slot-level simulation
proves (53 entries in six clusters, one of them over the table's end) before the GPU is asked."""
import copy
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import commit_revoke_worker as RW
from commit_log_model import COMMIT_CONFLICT, OK, REF_SELF
from commit_log_worker import h, ref
from commit_revoke_model import RevokeModel, TableSim
from corda_amd import _lib
from corda_amd._lib import lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ALICE, BOB = 7, 8


@pytest.fixture
def log(engine):
    lid = engine.commit_log_create(10, salt=bytes(range(16)))
    yield lid
    engine.commit_log_destroy(lid)


class Small:
    """The 64-slot log of commit_revoke_worker with its model, its simulation and its members."""

    def __init__(self, engine):
        self.engine, self.model, self.sim = engine, RevokeModel(), TableSim(6, RW.SALT)
        self.lid = engine.commit_log_create(6, salt=RW.SALT)
        self.members, self.rows = RW.fill_small_table(engine, self.lid, self.model, self.sim)
        self.universe = [r for refs in self.members.values() for r in refs]
        assert engine.commit_log_stats(self.lid)[:2] == (53, 64)

    def at(self, slot):
        r = self.sim.slots[slot]
        return (r, self.rows[r])

    def revoke(self, rows):
        state(self.engine, self.lid, self.model, self.universe, revoke=rows)
        for r in {r for r, by in rows if self.sim.slot_of(r) is not None and self.rows[r] == by}:
            self.sim.erase(r)
        assert self.sim.entries() == len(self.model.log)


@pytest.fixture
def small(engine):
    s = Small(engine)
    yield s
    engine.commit_log_destroy(s.lid)


def state(engine, lid, model, universe, revoke=None, commit=None, **kw):
    """One call through the GPU and the model, then the universe's lookup and the entry count."""
    out = None
    if revoke is not None:
        out = engine.commit_log_revoke(lid, revoke)
        assert out == model.revoke(revoke)
    if commit is not None:
        st, cm, rs, rb = engine.commit_inputs(lid, commit, **kw)
        out = model.commit_batch(commit, **kw)
        assert ([int(x) for x in st], [int(x) for x in cm], rs, rb) == tuple(out)
    assert engine.commit_log_lookup(lid, universe) == [model.log.get((bytes(r[0]), r[1])) for r in universe]
    entries, _, next_seq = engine.commit_log_stats(lid)
    assert (entries, next_seq) == (len(model.log), model.next_seq)
    return out


def exported(engine, lid, model, since=0):
    got = engine.commit_log_export(lid, since)
    assert sorted(got) == sorted(model.export(since))
    return got


# ---- 1. every outcome of a row in one call -----------------------------------------------------------
def test_every_outcome_in_one_call(engine, log):
    m, uni = RevokeModel(), [ref(i) for i in range(12)]
    loaded = [(ref(8), (h("old", 1), 3, BOB)), (ref(9), (h("old", 2), 0, ALICE))]
    assert engine.commit_log_load(log, loaded) == m.load(loaded) == 0
    state(engine, log, m, uni, commit=[(h("tx", 1), ALICE, [ref(0), ref(1)], None), (h("tx", 2), BOB, [ref(2)], None),
                                      (h("tx", 3), BOB, [ref(3), ref(4)], None)])
    rows = [(ref(0), (h("tx", 1), 0, ALICE)),                      # matches
            (ref(11), (h("tx", 1), 0, ALICE)),                     # absent ref
            (ref(1), (h("tx", 9), 1, ALICE)),                      # right ref, another id
            (ref(2), (h("tx", 2), 1, BOB)),                        # ... another position
            (ref(3), (h("tx", 3), 0, ALICE)),                      # ... another caller
            (ref(4), (h("tx", 3), 1, BOB)), (ref(4), (h("tx", 3), 1, BOB)), (ref(4), (h("tx", 3), 1, BOB)),
            (ref(8), (h("old", 1), 3, BOB))]                       # a loaded row
    assert state(engine, log, m, uni, revoke=rows) == ([1, 0, 0, 0, 0, 1, 1, 1, 1], 3)
    # the refused rows' entries are there unchanged
    assert engine.commit_log_lookup(log, [ref(1), ref(2), ref(3)]) == [
        (h("tx", 1), 1, ALICE), (h("tx", 2), 0, BOB), (h("tx", 3), 0, BOB)]
    assert engine.commit_log_lookup(log, [ref(0), ref(4), ref(8)]) == [None, None, None]


# ---- 2. wave and block edges ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_revoke_sizes(engine, log, n):
    """n rows over 300 loaded entries in 1024 slots: two in three match, the rest name another
    caller or an absent ref; every fifth row is the row before it once more."""
    rng = random.Random(n)
    m, uni = RevokeModel(), [ref(5000 + i) for i in range(320)]
    loaded = [(uni[i], (h("old", i), i % 4, i % 3)) for i in range(300)]
    assert engine.commit_log_load(log, loaded) == m.load(loaded) == 0
    rows = [loaded[0]]
    for i in rng.sample(range(1, 320), min(n, 319)):
        r, by = (uni[i], (h("old", i), i % 4, i % 3))
        rows.append((r, by if rng.random() < 2 / 3 else (by[0], by[1], by[2] + 1)))
        if len(rows) % 5 == 4:
            rows.append(rows[-1])
    rows = rows[:n]
    revoked, removed = state(engine, log, m, uni, revoke=rows)
    assert len(revoked) == n and 0 < removed <= sum(revoked) and (n < 63 or (0 in revoked and removed < sum(revoked)))
    exported(engine, log, m)


# ---- 3. cluster shapes, on the 64-slot table -----------------------------------------------------------
def test_first_and_last_slot_of_a_cluster(small):
    sim = small.sim
    assert sim.slots[44] is None and sim.slots[45] is not None            # 45: the first slot of D
    small.revoke([small.at(45)])
    assert sim.slots[52] is not None and sim.slots[53] is None            # 52: the last slot of E
    small.revoke([small.at(52)])
    exported(small.engine, small.lid, small.model)


def test_two_adjacent_and_a_whole_cluster(small):
    sim = small.sim
    assert sim.cluster_of(sim.slots[9]) == sim.cluster_of(sim.slots[10]) == list(range(7, 20))
    small.revoke([small.at(10), small.at(9)])
    whole = [small.at(s) for s in range(21, 30)]
    assert sim.slots[20] is None and sim.slots[30] is None and all(r is not None for r, _ in whole)
    random.Random(3).shuffle(whole)
    small.revoke(whole)
    assert all(s is None for s in sim.slots[20:31])


def test_a_later_entry_moves_two_positions_back(small):
    sim = small.sim
    probe = copy.deepcopy(sim)
    moves = probe.erase(sim.slots[32])
    assert 2 in [(f - t) % 64 for f, t in moves.values()] and all(31 <= f <= 43 for f, _ in moves.values())
    small.revoke([small.at(32)])


def test_the_cluster_over_the_tables_end(small):
    sim = small.sim
    assert sim.cluster_of(sim.slots[63]) == [58, 59, 60, 61, 62, 63, 0, 1, 2, 3, 4, 5]
    probe = copy.deepcopy(sim)
    crossed = [r for s in (60, 63, 0, 3) for r, (f, t) in probe.erase(sim.slots[s]).items() if f < t]
    assert crossed  # the simulation moves an entry from the table's first slots back to its last ones
    small.revoke([small.at(0), small.at(60), small.at(3), small.at(63)])
    exported(small.engine, small.lid, small.model)
    # what is left of it, then everything: the log is empty and takes the same rows again
    small.revoke([(r, small.rows[r]) for r in small.universe])
    assert small.model.log == {} and small.engine.commit_log_export(small.lid) == []
    rows = [(r, by) for r, by in small.rows.items()][:50]
    assert small.engine.commit_log_load(small.lid, rows) == small.model.load(rows) == 0
    state(small.engine, small.lid, small.model, small.universe)


# ---- 4. recommit ----------------------------------------------------------------------------------------
def test_recommit_after_a_revoke(engine, log):
    m, uni = RevokeModel(), [ref(i) for i in range(6)]
    req = (h("tx", 1), ALICE, [ref(0), ref(1)], None)
    rows = [(ref(0), (h("tx", 1), 0, ALICE)), (ref(1), (h("tx", 1), 1, ALICE))]
    assert state(engine, log, m, uni, commit=[req])[1] == [1]
    st, cm, rs, _ = state(engine, log, m, uni, commit=[req])
    assert (st, cm, rs) == ([OK], [0], [[REF_SELF, REF_SELF]])          # the retry: "nothing to persist"
    assert state(engine, log, m, uni, revoke=rows) == ([1, 1], 2)
    assert state(engine, log, m, uni, commit=[req])[1] == [1]            # committed again: rows to persist
    assert state(engine, log, m, uni, revoke=rows[1:]) == ([1], 1)
    st, cm, _, _ = state(engine, log, m, uni, commit=[(h("tx", 2), BOB, [ref(1), ref(2)], None),
                                                      (h("tx", 3), BOB, [ref(0)], None)])
    assert (st, cm) == ([OK, COMMIT_CONFLICT], [1, 0])                   # the freed ref is spent by another


def test_a_doubled_ref_is_revoked_by_its_last_position(engine, log):
    m, uni = RevokeModel(), [ref(i) for i in range(4)]
    req = (h("tx", 1), ALICE, [ref(0), ref(1), ref(0)], None)
    state(engine, log, m, uni, commit=[req])
    assert state(engine, log, m, uni, revoke=[(ref(0), (h("tx", 1), 0, ALICE))]) == ([0], 0)
    assert state(engine, log, m, uni, revoke=[(ref(0), (h("tx", 1), 2, ALICE)), (ref(1), (h("tx", 1), 1, ALICE))]) == \
        ([1, 1], 2)
    assert state(engine, log, m, uni, commit=[req])[1] == [1]


# ---- 5. dense interleaving ------------------------------------------------------------------------------
def test_dense_commits_and_revokes_equal_the_model(engine):
    want = RW.model_dense()
    assert RW.engine_dense(engine) == want
    revokes = [res for kind, res, _, _ in want if kind == "revoke"]
    assert sum(r[1] for r in revokes) > 20 and any(0 in r[0] for r in revokes)  # removals, and stale rows refused


def test_dense_interleaving_with_the_sweep_alone():
    """Once more in a process of its own with CORDAHIP_COMMIT_ROUNDS=0."""
    env = dict(os.environ, CORDAHIP_COMMIT_ROUNDS="0")
    p = subprocess.run([sys.executable, os.path.join(HERE, "commit_revoke_worker.py")], capture_output=True, text=True,
                       env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == RW.model_dense()


# ---- 6. reserve -----------------------------------------------------------------------------------------
def test_reserve_after_a_revoke_and_revoke_after_a_reserve(small):
    eng, lid = small.engine, small.lid
    small.revoke([small.at(s) for s in (59, 62, 1, 8, 33)])
    eng.commit_log_reserve(lid, 9)   # the rehash copies the padding: it must meet no mark
    state(eng, lid, small.model, small.universe)
    assert eng.commit_log_stats(lid)[1] == 512
    rows = [(r, by) for r, by in small.rows.items() if r in small.model.log][::2]
    assert state(eng, lid, small.model, small.universe, revoke=rows) == ([1] * len(rows), len(rows))
    exported(eng, lid, small.model)
    rows = [(r, small.rows[r]) for r in small.model.log]
    state(eng, lid, small.model, small.universe, revoke=rows)
    assert eng.commit_log_export(lid) == [] and eng.commit_log_stats(lid)[0] == 0


# ---- 7. ordering ----------------------------------------------------------------------------------------
def test_a_revoke_takes_its_turn_behind_a_ticket(engine, log):
    m, uni = RevokeModel(), [ref(i) for i in range(40)]
    txs = [(h("ord", t), ALICE, [ref(2 * t), ref(2 * t + 1)], None) for t in range(20)]
    rows = [(ref(2 * t + i), (h("ord", t), i, ALICE)) for t in range(20) for i in range(2)]
    ticket = engine.commit_inputs_submit(log, txs)
    got = engine.commit_log_revoke(log, rows)   # at once, the ticket not waited for
    st, cm, rs, rb = ticket.wait()
    assert ([int(x) for x in st], [int(x) for x in cm], rs, rb) == tuple(m.commit_batch(txs)) and all(cm)
    assert got == m.revoke(rows) == ([1] * 40, 40)
    state(engine, log, m, uni)
    assert exported(engine, log, m) == []


# ---- 8. export ------------------------------------------------------------------------------------------
def test_export_equals_the_model(engine, log):
    m, uni = RevokeModel(), [ref(i) for i in range(40)]
    assert exported(engine, log, m) == []
    loaded = [(ref(30 + i), (h("old", i), i, BOB)) for i in range(8)]
    assert engine.commit_log_load(log, loaded) == m.load(loaded)
    assert {s for _, _, s in exported(engine, log, m)} == {0}
    first = [(h("a", t), ALICE, [ref(2 * t), ref(2 * t + 1)], None) for t in range(5)]
    state(engine, log, m, uni, commit=first)
    base = engine.commit_log_stats(log)[2]
    second = [(h("b", 0), BOB, [ref(0)], None), (h("b", 1), BOB, [], None), (h("b", 2), BOB, [ref(12), ref(13)], None),
              (h("b", 3), BOB, [ref(14), ref(14)], None)]
    state(engine, log, m, uni, commit=second)
    assert sorted(exported(engine, log, m, base)) == sorted([
        (ref(12), (h("b", 2), 0, BOB), base + 2), (ref(13), (h("b", 2), 1, BOB), base + 2),
        (ref(14), (h("b", 3), 1, BOB), base + 3)])  # the second batch's insertions, seq == base + t
    state(engine, log, m, uni, revoke=[(ref(13), (h("b", 2), 1, BOB)), (ref(3), (h("a", 1), 1, ALICE)),
                                       (ref(31), (h("old", 1), 1, BOB))])
    assert len(exported(engine, log, m)) == 8 + 10 + 3 - 3
    assert len(exported(engine, log, m, base)) == 2
    assert exported(engine, log, m, base + 4) == []


def test_export_into_a_short_buffer_and_the_counting_call(engine, log):
    m = RevokeModel()
    loaded = [(ref(i), (h("old", i), i, BOB)) for i in range(100)]
    assert engine.commit_log_load(log, loaded) == m.load(loaded)
    total = ctypes.c_uint64(77)
    assert lib().cordahip_commit_log_export(engine.ctx, log, 0, None, None, 0, ctypes.byref(total)) == 0
    assert total.value == 100                                            # the counting call
    cap, guard = 37, 3
    rows = np.full(cap + guard, 0xA5, dtype=np.uint8).repeat(76).view(_lib.COMMIT_ROW_DTYPE)
    seq = np.full(cap + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert lib().cordahip_commit_log_export(engine.ctx, log, 0, rows.ctypes.data, seq.ctypes.data, cap,
                                            ctypes.byref(total)) == 0
    assert total.value == 100                                            # exact, though only cap rows fit
    got = [((bytes(r["ref"]["txhash"]), int(r["ref"]["index"])),
            (bytes(r["by"]["id"]), int(r["by"]["input_index"]), int(r["by"]["caller"]))) for r in rows[:cap]]
    assert len(set(got)) == cap and all(m.log.get(r) == by for r, by in got) and not seq[:cap].any()
    assert rows[cap:].tobytes() == b"\xa5" * (76 * guard) and (seq[cap:] == 0xA5A5A5A5A5A5A5A5).all()
    # rows without seq
    assert lib().cordahip_commit_log_export(engine.ctx, log, 0, rows.ctypes.data, None, cap + guard,
                                            ctypes.byref(total)) == 0
    assert total.value == 100 and len({bytes(r["ref"]["txhash"]) + bytes(r["by"]["id"]) for r in rows}) == cap + guard


# ---- 9. arguments ---------------------------------------------------------------------------------------
def test_arguments(engine):
    lid = engine.commit_log_create(6)
    row, rev, n = _lib.CommitRow(), ctypes.c_uint8(9), ctypes.c_uint64(9)
    L = lib()
    assert L.cordahip_commit_log_revoke(engine.ctx, lid, None, 0, None, None) == 0         # n = 0: a no-op
    assert L.cordahip_commit_log_revoke(engine.ctx, lid, None, 0, None, ctypes.byref(n)) == 0 and n.value == 0
    assert engine.commit_log_revoke(lid, []) == ([], 0) and engine.commit_log_export(lid) == []
    for bad in (lid + 1000, 0):
        assert L.cordahip_commit_log_revoke(engine.ctx, bad, ctypes.byref(row), 1, ctypes.byref(rev), None) == -1
        assert L.cordahip_commit_log_export(engine.ctx, bad, 0, None, None, 0, ctypes.byref(n)) == -1
    assert L.cordahip_commit_log_revoke(engine.ctx, lid, None, 1, ctypes.byref(rev), None) == -1
    assert L.cordahip_commit_log_revoke(engine.ctx, lid, ctypes.byref(row), 1, None, None) == -1
    assert L.cordahip_commit_log_export(engine.ctx, lid, 0, None, None, 1, ctypes.byref(n)) == -1
    assert L.cordahip_commit_log_export(engine.ctx, lid, 0, None, None, 0, None) == -1
    engine.commit_log_destroy(lid)
    assert L.cordahip_commit_log_revoke(engine.ctx, lid, ctypes.byref(row), 1, ctypes.byref(rev), None) == -1
    assert L.cordahip_commit_log_export(engine.ctx, lid, 0, None, None, 0, ctypes.byref(n)) == -1
    assert rev.value == 9


# ---- 10. the notary flow with the database write inside ---------------------------------------------------
def test_a_failed_write_is_revoked_and_nothing_is_released(engine, oracle):
    from corda_amd import resolve as R
    cases = json.load(open(os.path.join(HERE, "golden", "pmt_vectors.json")))["cases"]
    by_root = {}
    for c in cases:
        if c["status"] == 0:
            by_root.setdefault(c["root"], ([bytes.fromhex(x) for x in c["leaves"]],
                                           [(t, bytes.fromhex(hh) if hh else None) for t, hh in c["tokens"]],
                                           bytes.fromhex(c["root"])))
    ftxs = list(by_root.values())[:4]
    assert len(ftxs) == 4
    inputs = [[ref(0), ref(1)], [ref(1), ref(2)], [ref(3), ref(3)], [ref(20)]]
    callers, now, tol = [ALICE, BOB, BOB, ALICE], 10 ** 18, 10 ** 9
    seed = hashlib.sha256(b"notary-key-3").digest()
    kid, _ = engine.signer_add_ed25519(seed)
    lid = engine.commit_log_create(8)
    try:
        m, uni = RevokeModel(), [ref(i) for i in range(24)]
        old = [(ref(20), (h("old", 0), 0, BOB))]
        assert engine.commit_log_load(lid, old) == m.load(old)
        seen = []

        class WriteFailed(Exception):
            pass

        def failing(rows):
            seen.append(list(rows))
            raise WriteFailed()
        with pytest.raises(WriteFailed):
            R.notarise_filtered_transactions_persisted(engine, lid, ftxs, inputs, [None] * 4, callers, kid, now, tol,
                                                       failing)
        want_rows = [(ref(0), (ftxs[0][2], 0, ALICE)), (ref(1), (ftxs[0][2], 1, ALICE)), (ref(3), (ftxs[2][2], 1, BOB))]
        assert seen == [want_rows]
        m.next_seq += 4  # the call consumed its sequence numbers; nothing else is left of it
        state(engine, lid, m, uni)
        exported(engine, lid, m)
        answers, rows = R.notarise_filtered_transactions_persisted(engine, lid, ftxs, inputs, [None] * 4, callers, kid,
                                                                   now, tol, seen.append)
        assert rows == want_rows == seen[1]
        sig_buf, pub_buf = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)
        for t in (0, 2):
            oracle.oracle_ed25519_sign(seed, ftxs[t][2], 32, pub_buf, sig_buf)
            assert answers[t] == sig_buf.raw
        assert answers[1] == R.NotaryError("Conflict", ftxs[1][2], {ref(1): (ftxs[0][2], 1, ALICE)})
        assert answers[3] == R.NotaryError("Conflict", ftxs[3][2], {ref(20): (h("old", 0), 0, BOB)})
        m.load(rows)
        assert engine.commit_log_lookup(lid, uni) == [m.log.get(r) for r in uni]
    finally:
        engine.commit_log_destroy(lid)
        engine.signer_remove(kid)
