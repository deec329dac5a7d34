"""Shared pieces of tests/test_gpu_commit_revoke.py: the 64-slot table whose cluster shapes the
tests rely on, and the dense commit / revoke interleaving as a function and as a program --
`python tests/commit_revoke_worker.py` runs it on a fresh engine under whatever
CORDAHIP_COMMIT_ROUNDS the environment sets and prints one JSON line with every output."""
import json
import os
import random
import sys

from commit_log_worker import UNIVERSE, h, ref
from commit_revoke_model import RevokeModel, TableSim

HERE = os.path.dirname(os.path.abspath(__file__))
SALT = bytes(range(100, 116))
# (first slot, entries) of the clusters of the 64-slot table: 53 entries, one empty slot between
# neighbours, the first cluster running over the table's end (58..63, 0..5)
CLUSTERS = {"W": (58, 12), "A": (7, 13), "B": (21, 9), "C": (31, 13), "D": (45, 3), "E": (50, 3)}


def _offset(k):
    """Home of a cluster's k-th entry, relative to the cluster's first slot: the even entries lie at
    home (a removal before them leaves them where they are), the odd ones up to four slots past
    theirs (and are shifted over the ones that stay)."""
    return k if k % 2 == 0 else max(0, k - 4)


def small_table_plan():
    """[[(cluster name, ref)]]: call k holds the k-th entry of every cluster that has one. The
    entries of one call lie in different clusters, so one call may insert them in any order; the
    calls in sequence put the k-th entry of a cluster that begins at slot a into slot a + k."""
    sim = TableSim(6, SALT)
    by_home, i = {}, 0
    while min((len(by_home.get(s, [])) for s in range(64)), default=0) < 4:
        r = (h("small", i), i % 3)
        by_home.setdefault(sim.home(r), []).append(r)
        i += 1
    plan = []
    for k in range(max(n for _, n in CLUSTERS.values())):
        plan.append([(name, by_home[(a + _offset(k)) % 64].pop()) for name, (a, n) in CLUSTERS.items() if k < n])
    return plan


def fill_small_table(engine, lid, model, sim):
    """The plan through the GPU, the model and the simulation: even calls are loads (sequence
    number 0), odd calls commit one single-input transaction per ref. Returns {cluster: [refs in
    slot order]} and the rows as they would be persisted, {ref: by}."""
    members = {name: [] for name in CLUSTERS}
    for k, call in enumerate(small_table_plan()):
        refs = [r for _, r in call]
        if k % 2 == 0:
            rows = [(r, (h("loaded", k), j, 9)) for j, r in enumerate(refs)]
            assert engine.commit_log_load(lid, rows) == model.load(rows) == 0
        else:
            txs = [(h("fill-%d" % k, j), j % 3, [r], None) for j, r in enumerate(refs)]
            st, cm, _, _ = engine.commit_inputs(lid, txs)
            want = model.commit_batch(txs)
            assert ([int(x) for x in st], [int(x) for x in cm]) == (want[0], want[1]) and all(want[1])
        for name, r in call:
            a, _ = CLUSTERS[name]
            assert sim.put(r) == (a + len(members[name])) % 64, (name, k)
            members[name].append(r)
    assert sorted(map(tuple, sim.clusters())) == sorted(
        tuple((a + q) % 64 for q in range(n)) for a, n in CLUSTERS.values())
    return members, dict(model.log)


# ---- the dense interleaving ---------------------------------------------------------------------
def dense_steps(seed=20261020, ntx=23, nsteps=8):
    """Commit batches over commit_log_worker's universe (40 refs, 8 ids, 3 callers) alternating
    with revokes. What a revoke names depends on the commits' outcomes, so the steps are drawn while
    the model runs: yields ("commit", txs) and ("revoke", rows), rows a random subset of what the
    batch before committed plus rows that earlier revokes or later commits have made stale."""
    rng = random.Random(seed)
    model, stale = RevokeModel(), []
    for _ in range(nsteps):
        txs = [(h("tx", rng.randrange(8)), rng.randrange(3),
                [ref(rng.randrange(UNIVERSE)) for _ in range(rng.randrange(5))], None) for _ in range(ntx)]
        before = dict(model.log)
        model.commit_batch(txs)
        yield "commit", txs
        fresh = [(r, by) for r, by in model.log.items() if before.get(r) != by]
        rows = [row for row in fresh if rng.random() < 0.6] + [row for row in stale if rng.random() < 0.3]
        rows += [rows[0]] * 2 if rows else []
        rng.shuffle(rows)
        model.revoke(rows)
        stale += rows
        yield "revoke", rows


def _plain_by(b):
    return None if b is None else [b[0].hex(), b[1], b[2]]


def run_dense(target, lookup, entries):
    """The steps through `target` (an Engine bound to a log, or the model): every output, and after
    every step the universe's lookup and the entry count, in a JSON-able form."""
    out = []
    for kind, arg in dense_steps():
        if kind == "commit":
            st, cm, rs, rb = target.commit(arg)
            res = [[int(x) for x in st], [int(x) for x in cm], rs, [[_plain_by(b) for b in row] for row in rb]]
        else:
            revoked, removed = target.revoke(arg)
            res = [list(revoked), removed]
        out.append([kind, res, entries(), [_plain_by(b) for b in lookup([ref(i) for i in range(UNIVERSE)])]])
    return out


class _OnEngine:
    def __init__(self, engine, lid):
        self.commit = lambda txs: engine.commit_inputs(lid, txs)
        self.revoke = lambda rows: engine.commit_log_revoke(lid, rows)


class _OnModel:
    def __init__(self, m):
        self.commit = m.commit_batch
        self.revoke = m.revoke


def engine_dense(engine):
    lid = engine.commit_log_create(10)
    try:
        return run_dense(_OnEngine(engine, lid), lambda refs: engine.commit_log_lookup(lid, refs),
                         lambda: engine.commit_log_stats(lid)[0])
    finally:
        engine.commit_log_destroy(lid)


def model_dense():
    m = RevokeModel()
    return run_dense(_OnModel(m), lambda refs: [m.log.get(r) for r in refs], lambda: len(m.log))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from corda_amd.engine import Engine
    with Engine(1) as eng:
        print(json.dumps(engine_dense(eng)))
