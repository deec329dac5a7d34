"""FilteredTransaction build on one GPU: cordahip_filtered_tx_build_device (K3 leaf hashes + K10
pmt_build_kernel) on bench.py's c4 corpus resident in HBM (cash-issue transactions, five leaves
each), with a NotaryFlow-like mask: one component in five selected (--flag-leaf, default the
third), so each tear-off is an 8-position padded tree cut down to a few tokens. Slots have the
exact bound (15 tokens a transaction). Device events on the workload's stream, >= 20 steps after
warm-up. The tool also makes the workload's own device signed-tx call (K3 + K4 merkle_root_kernel
+ the signatures) over the same leaves, before and after the timed steps, so a kernel-trace run
of this tool shows merkle_root_kernel beside pmt_build_kernel on the same leaves. Prints ONE JSON
line:
  build_ms              the build call, median step (min / max beside it), and txs_per_s
  ids_match             the ids the build wrote equal the signed-tx call's
  statuses, tokens_per_tx   what the build reported (all OK, the same count in every transaction)
  out_bytes_per_tx      bytes the call writes per transaction that a reader needs: id, status,
                        count, and 33 B per token written; slot_bytes_per_tx: the slots' size
  verified              a sample of the built tear-offs through cordahip_filtered_tx_verify: all OK
A run without a GPU fails; nothing falls back.
  python tools/pmt_build_bench.py [--txs 1250000] [--steps 20] [--warmup 3] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txs", type=int, default=10_000_000 // 8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flag-leaf", type=int, default=2)
    ap.add_argument("--verify-sample", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("pmt_build_bench.py: no GPU", file=sys.stderr)
        return 2
    import bench
    from corda_amd import _lib
    from corda_amd.engine import Engine

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    res = {"workload": "filtered_tx_build_device (c4 corpus in HBM, one leaf in five flagged)", "steps": a.steps,
           "warmup": a.warmup}
    with Engine(1) as eng:
        w = bench.C4(eng, dev, stream, 0, bench.parse_args(["--workload", "c4", "--c4-txs", str(a.txs)]))
        ntx = w.ntx
        nl = (w.leaf_off.shape[0] - 1) // ntx
        bound = _lib.pmt_slot_bound(nl)
        include = torch.zeros(ntx * nl, dtype=torch.uint8, device=dev)
        include[a.flag_leaf % nl::nl] = 1
        tko = torch.arange(ntx + 1, dtype=torch.int64, device=dev) * bound
        txid = torch.empty((ntx, 32), dtype=torch.uint8, device=dev)
        tok = torch.empty(ntx * bound, dtype=torch.uint8, device=dev)
        th = torch.empty((ntx * bound, 32), dtype=torch.uint8, device=dev)
        cnt = torch.empty(ntx, dtype=torch.int64, device=dev)
        st = torch.empty(ntx, dtype=torch.uint8, device=dev)

        def build():
            eng.filtered_tx_build_device(w.leaf_bytes, w.leaf_off, w.tx_leaf_off, include, tko, txid, tok, th, cnt, st,
                                         stream=stream)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        w.step()  # the existing signed-tx call over the same leaves (K3, K4, signatures)
        for _ in range(a.warmup):
            build()
        stream.synchronize()
        ms = [timed(build) for _ in range(a.steps)]
        w.step()
        stream.synchronize()
        m = float(np.median(ms))
        counts = cnt.cpu().numpy()
        status = st.cpu().numpy()
        ntok = int(counts.sum())
        res.update({"txs": ntx, "leaves_per_tx": nl, "slot_tokens": bound, "build_ms": m, "build_ms_min": min(ms),
                    "build_ms_max": max(ms), "txs_per_s": ntx / (m * 1e-3),
                    "ids_match": bool(torch.equal(txid, w.txid)),
                    "statuses": {str(k): int(v) for k, v in zip(*np.unique(status, return_counts=True))},
                    "tokens_per_tx": ntok / ntx, "tokens_per_tx_min": int(counts.min()),
                    "tokens_per_tx_max": int(counts.max()),
                    "out_bytes_per_tx": 32 + 1 + 8 + 33.0 * ntok / ntx, "slot_bytes_per_tx": 33 * bound})
        # a sample of the tear-offs through the receiver's call
        n = min(a.verify_sample, ntx)
        lo = w.leaf_off[:n * nl + 1].cpu().numpy()
        lb = w.leaf_bytes[:int(lo[-1])].cpu().numpy()
        tk, hh, ids = tok[:n * bound].cpu().numpy(), th[:n * bound].cpu().numpy(), txid[:n].cpu().numpy()
        f = a.flag_leaf % nl
        ftxs = []
        for t in range(n):
            leaf = lb[int(lo[t * nl + f]):int(lo[t * nl + f + 1])].tobytes()
            toks = [(int(tk[k]), None if tk[k] == 2 else hh[k].tobytes())
                    for k in range(t * bound, t * bound + int(counts[t]))]
            ftxs.append(([leaf], toks, ids[t].tobytes()))
        got = eng.filtered_tx_verify(ftxs)
        res["verified"] = {"sample": n, "ok": int((got == 0).sum())}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    good = res["ids_match"] and res["statuses"] == {"0": ntx} and res["verified"]["ok"] == n
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
