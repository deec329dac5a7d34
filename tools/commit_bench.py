"""Device time of the notary commit log's batched commit (K16, cordahip_commit_inputs_device)
at several CORDAHIP_COMMIT_ROUNDS settings: the library reads the variable once, so every
setting runs in a child process of its own (`--child`), and the parent prints one JSON line.

Workload: `--ntx` transactions of `--inputs` inputs each, refs drawn from a universe of
`--universe` values (so a few per cent of the transactions meet a ref another transaction of
the batch, or an earlier batch, consumed), `--batches` consecutive batches on one log of
2^`--log2` slots. Per setting: the median ms per batch (HIP events around the call), the
transactions per second that is, and the committed / conflict counts, which must not depend
on the setting.

  python tools/commit_bench.py --rounds 0,1,2,3 --out profiles/commit_rounds.json

`--revoke` and `--export` measure cordahip_commit_log_revoke and cordahip_commit_log_export
instead, each in one child process at the default round count, on a log of 2^`--log2` slots
loaded to `--fill` of its capacity. Both are host forms, so their figures are wall-clock ms of
the C call (stage copies and the wait included), median of `--batches` repeats; the commit
line next to them is the device time of cordahip_commit_inputs_device, as above.
  --revoke: per repeat, one batch of `--ntx` transactions of `--inputs` fresh inputs is
            committed, all its rows are revoked, the batch is committed again and
            `--few` of its rows are revoked (then the rest, untimed).
  --export: the export of the whole log, and of one batch's insertions by since_seq.

  python tools/commit_bench.py --revoke --export --log2 24,20 --out profiles/commit_revoke.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import numpy as np
    import torch

    from corda_amd.engine import Engine
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    ms, committed, conflicts = [], 0, 0
    with Engine(1) as eng:
        log = eng.commit_log_create(a.log2, salt=bytes(16))
        n, k = a.ntx, a.inputs
        off = torch.arange(0, (n + 1) * k, k, dtype=torch.int64, device=dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        cm = torch.empty(n, dtype=torch.uint8, device=dev)
        rs = torch.empty(n * k, dtype=torch.uint8, device=dev)
        rb = torch.empty((n * k, 40), dtype=torch.uint8, device=dev)
        for b in range(a.batches + 1):  # batch 0 warms up (scratch growth, code load)
            refs = np.zeros((n * k, 36), np.uint8)
            refs[:, :8] = rng.integers(0, a.universe, n * k, dtype=np.uint64).view(np.uint8).reshape(-1, 8)
            txid = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            d_refs, d_txid = torch.from_numpy(refs).to(dev), torch.from_numpy(txid).to(dev)
            d_caller = torch.zeros(n, dtype=torch.int32, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s = torch.cuda.current_stream()
            e0.record(s)
            eng.commit_inputs_device(log, d_txid, d_caller, d_refs, off, st, cm, rs, rb, stream=s)
            e1.record(s)
            e1.synchronize()
            if b:
                ms.append(e0.elapsed_time(e1))
                committed += int(cm.sum().item())
                conflicts += int((st == 16).sum().item())
            eng.commit_log_stats(log)
        entries = eng.commit_log_stats(log)[0]
        eng.commit_log_destroy(log)
    ms.sort()
    med = ms[len(ms) // 2]
    print(json.dumps({"rounds": os.environ.get("CORDAHIP_COMMIT_ROUNDS", "default"), "ms_per_batch": round(med, 3),
                      "ms_all": [round(x, 3) for x in ms], "tx_per_s": round(a.ntx / med * 1e3),
                      "committed": committed, "conflicts": conflicts, "entries": entries}))


def _median(xs):
    return round(sorted(xs)[len(xs) // 2], 3)


def child_revoke_export(a):
    import ctypes
    import time

    import numpy as np
    import torch

    from corda_amd import _lib
    from corda_amd.engine import Engine
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    L = _lib.lib()
    n, k = a.ntx, a.inputs
    out = {"log2": int(a.log2), "fill": a.fill}

    def fresh_rows(count):
        """`count` rows with random 32-byte hashes, as bytes [count, 76]."""
        rows = np.zeros((count, 76), np.uint8)
        rows[:, :32] = rng.integers(0, 256, (count, 32), dtype=np.uint8)
        return rows

    def timed(f):
        t0 = time.perf_counter()
        rc = f()
        ms = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        return ms

    with Engine(1) as eng:
        log = eng.commit_log_create(int(a.log2), salt=bytes(16))
        target = int(a.fill * (1 << int(a.log2)))
        dup = ctypes.c_uint64()
        for at in range(0, target, 1 << 20):  # loaded a million rows at a time: the stage stays small
            rows = fresh_rows(min(1 << 20, target - at))
            assert L.cordahip_commit_log_load(eng.ctx, log, rows.ctypes.data, len(rows), ctypes.byref(dup)) == 0
        out["loaded"] = eng.commit_log_stats(log)[0]
        off = torch.arange(0, (n + 1) * k, k, dtype=torch.int64, device=dev)
        st = torch.empty(n, dtype=torch.uint8, device=dev)
        cm = torch.empty(n, dtype=torch.uint8, device=dev)
        rs = torch.empty(n * k, dtype=torch.uint8, device=dev)
        rb = torch.empty((n * k, 40), dtype=torch.uint8, device=dev)
        d_caller = torch.zeros(n, dtype=torch.int32, device=dev)
        revoked = np.zeros(n * k, np.uint8)
        removed, total = ctypes.c_uint64(), ctypes.c_uint64()

        def commit(rows):
            """The batch whose persisted rows are `rows` (caller 0, position i of k); device ms."""
            d_refs = torch.from_numpy(np.ascontiguousarray(rows[:, :36])).to(dev)
            d_txid = torch.from_numpy(np.ascontiguousarray(rows[::k, 36:68])).to(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s = torch.cuda.current_stream()
            e0.record(s)
            eng.commit_inputs_device(log, d_txid, d_caller, d_refs, off, st, cm, rs, rb, stream=s)
            e1.record(s)
            e1.synchronize()
            assert int(cm.sum().item()) == n
            return e0.elapsed_time(e1)

        def revoke(rows):
            m = len(rows)
            ms = timed(lambda: L.cordahip_commit_log_revoke(eng.ctx, log, rows.ctypes.data, m, revoked.ctypes.data,
                                                            ctypes.byref(removed)))
            assert removed.value == m and revoked[:m].all()
            return ms

        def batch_rows():
            rows = fresh_rows(n * k)
            rows[:, 36:68] = np.repeat(rng.integers(0, 256, (n, 32), dtype=np.uint8), k, axis=0)
            rows[:, 68:72] = np.tile(np.arange(k, dtype=np.uint32), n).view(np.uint8).reshape(-1, 4)
            return rows

        if a.revoke:
            c_ms, all_ms, few_ms = [], [], []
            for b in range(a.batches + 1):  # repeat 0 warms up
                rows = batch_rows()
                c = commit(rows)
                r_all = revoke(rows)
                commit(rows)  # committed = 1 again: the log is as if the batch had never been there
                pick = rng.choice(n * k, a.few, replace=False)
                r_few = revoke(np.ascontiguousarray(rows[pick]))
                keep = np.ones(n * k, bool)
                keep[pick] = False
                revoke(np.ascontiguousarray(rows[keep]))
                eng.commit_log_stats(log)  # tightens the host's bound of the load
                if b:
                    c_ms.append(c), all_ms.append(r_all), few_ms.append(r_few)
            assert eng.commit_log_stats(log)[0] == out["loaded"]
            out["revoke"] = {"commit_device_ms": _median(c_ms), "rows": n * k, "revoke_all_wall_ms": _median(all_ms),
                             "revoke_all_wall_ms_all": [round(x, 3) for x in all_ms], "few": a.few,
                             "revoke_few_wall_ms": _median(few_ms),
                             "revoke_few_wall_ms_all": [round(x, 3) for x in few_ms]}
        if a.export:
            base = eng.commit_log_stats(log)[2]
            commit(batch_rows())
            entries = eng.commit_log_stats(log)[0]
            rows = np.zeros((entries, 76), np.uint8)
            seq = np.zeros(entries, np.uint64)
            whole, part, count = [], [], []
            for b in range(a.batches + 1):
                w = timed(lambda: L.cordahip_commit_log_export(eng.ctx, log, 0, rows.ctypes.data, seq.ctypes.data,
                                                               entries, ctypes.byref(total)))
                assert total.value == entries
                c = timed(lambda: L.cordahip_commit_log_export(eng.ctx, log, 0, None, None, 0, ctypes.byref(total)))
                q = timed(lambda: L.cordahip_commit_log_export(eng.ctx, log, base, rows.ctypes.data, seq.ctypes.data,
                                                               entries, ctypes.byref(total)))
                assert total.value == n * k and (seq[:n * k] >= base).all()
                if b:
                    whole.append(w), part.append(q), count.append(c)
            out["export"] = {"entries": entries, "whole_wall_ms": _median(whole), "count_only_wall_ms": _median(count),
                             "since_seq_rows": n * k, "since_seq_wall_ms": _median(part)}
        eng.commit_log_destroy(log)
    print(json.dumps(out))


def main_revoke_export(a):
    rows = []
    for log2 in a.log2.split(","):
        args = [sys.executable, os.path.abspath(__file__), "--child", "--log2=%s" % log2] + [
            "--%s=%s" % (k, getattr(a, k)) for k in ("ntx", "inputs", "batches", "seed", "fill", "few")] + [
            f for f in ("--revoke", "--export") if getattr(a, f[2:])]
        q = subprocess.run(args, capture_output=True, text=True, timeout=900)
        if q.returncode != 0:
            sys.stderr.write(q.stderr[-2000:])
            return 1
        rows.append(json.loads(q.stdout.strip().splitlines()[-1]))
    line = json.dumps({"workload": {k: getattr(a, k) for k in ("ntx", "inputs", "batches", "seed", "fill", "few")},
                       "logs": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--revoke", action="store_true")
    p.add_argument("--export", action="store_true")
    p.add_argument("--fill", type=float, default=0.5)
    p.add_argument("--few", type=int, default=64)
    p.add_argument("--rounds", default="0,1,2,3")
    p.add_argument("--ntx", type=int, default=1 << 16)
    p.add_argument("--inputs", type=int, default=2)
    p.add_argument("--universe", type=int, default=1 << 22)
    p.add_argument("--log2", default="21")
    p.add_argument("--batches", type=int, default=5)
    p.add_argument("--seed", type=int, default=20261020)
    p.add_argument("--out", default=None)
    p.add_argument("--child", action="store_true")
    a = p.parse_args()
    if a.revoke or a.export:
        return child_revoke_export(a) if a.child else main_revoke_export(a)
    a.log2 = int(a.log2)
    if a.child:
        return child(a)
    rows = []
    for r in a.rounds.split(","):
        env = dict(os.environ, CORDAHIP_COMMIT_ROUNDS=r)
        args = [sys.executable, os.path.abspath(__file__), "--child"] + [
            "--%s=%s" % (k, getattr(a, k)) for k in ("ntx", "inputs", "universe", "log2", "batches", "seed")]
        q = subprocess.run(args, capture_output=True, text=True, env=env, timeout=600)
        if q.returncode != 0:
            sys.stderr.write(q.stderr[-2000:])
            return 1
        rows.append(json.loads(q.stdout.strip().splitlines()[-1]))
    same = len({(r["committed"], r["conflicts"], r["entries"]) for r in rows}) == 1
    res = {"workload": {k: getattr(a, k) for k in ("ntx", "inputs", "universe", "log2", "batches", "seed")},
           "settings": rows, "results_independent_of_rounds": same}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
