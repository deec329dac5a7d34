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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", default="0,1,2,3")
    p.add_argument("--ntx", type=int, default=1 << 16)
    p.add_argument("--inputs", type=int, default=2)
    p.add_argument("--universe", type=int, default=1 << 22)
    p.add_argument("--log2", type=int, default=21)
    p.add_argument("--batches", type=int, default=5)
    p.add_argument("--seed", type=int, default=20261020)
    p.add_argument("--out", default=None)
    p.add_argument("--child", action="store_true")
    a = p.parse_args()
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
