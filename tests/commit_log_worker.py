"""The dense-collision parity batches of tests/test_gpu_commit_log.py as a function, and as a
program: `python tests/commit_log_worker.py` runs them on a fresh engine under whatever
CORDAHIP_COMMIT_ROUNDS the environment sets and prints one JSON line with every output, which
the test compares with the model's (round counts must not change a single byte)."""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NTX = (0, 1, 2, 63, 64, 65, 300)
UNIVERSE = 40


def h(tag, i=0):
    return hashlib.sha256(b"%s-%d" % (tag.encode(), i)).digest()


def ref(i):
    return (h("state", i // 2), i % 2)  # pairs of refs share a transaction hash


def dense_batches(ntx, seed=20261020):
    """Six consecutive batches of ntx transactions: 0-5 inputs from 40 refs, 8 ids, 3 callers;
    one request in six is an earlier one sent again (the retry path)."""
    rng = random.Random(seed * 1000 + ntx)
    out, sent = [], []
    for _ in range(6):
        batch = []
        for _ in range(ntx):
            if sent and rng.random() < 1 / 6:
                tx = rng.choice(sent)
            else:
                tx = (h("tx", rng.randrange(8)), rng.randrange(3),
                      [ref(rng.randrange(UNIVERSE)) for _ in range(rng.randrange(6))], None)
            batch.append(tx)
            sent.append(tx)
        out.append(batch)
    return out


def plain(res):
    st, cm, rs, rb = res
    return [[int(x) for x in st], [int(x) for x in cm], rs,
            [[None if b is None else [b[0].hex(), b[1], b[2]] for b in row] for row in rb]]


def run_dense(engine, ntx):
    """The six batches on a fresh 2^10-slot log: per batch the call's outputs and the lookup of
    the whole universe afterwards, in a JSON-able form."""
    log = engine.commit_log_create(10)
    out = []
    try:
        for txs in dense_batches(ntx):
            res = plain(engine.commit_inputs(log, txs))
            entries = engine.commit_log_stats(log)[0]  # also tightens the host's bound of the load
            look = engine.commit_log_lookup(log, [ref(i) for i in range(UNIVERSE)])
            out.append([res, entries, [None if b is None else [b[0].hex(), b[1], b[2]] for b in look]])
    finally:
        engine.commit_log_destroy(log)
    return out


def model_dense(ntx):
    from commit_log_model import CommitLogModel
    m = CommitLogModel()
    out = []
    for txs in dense_batches(ntx):
        res = plain(m.commit_batch(txs))
        look = [m.log.get(ref(i)) for i in range(UNIVERSE)]
        out.append([res, len(m.log), [None if b is None else [b[0].hex(), b[1], b[2]] for b in look]])
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    from corda_amd.engine import Engine
    with Engine(1) as eng:
        print(json.dumps({str(n): run_dense(eng, n) for n in NTX}))
