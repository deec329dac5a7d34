"""Required-signer coverage on one GPU: what tx_cover_kernel (cordahip_tx_cover_device) adds
to the device-resident signed-tx call, on bench.py's c4 corpus resident in HBM (cash-issue
transactions, 1-3 Ed25519 signers; each transaction's one required key is its first signer's
key, a single leaf). Device events on the workload's stream, >= 20 steps after warm-up, the
legs that are compared alternating step by step. Prints ONE JSON line:
  baseline_ms           cordahip_signed_tx_verify_ed25519_device alone (the code of the parent
                        commit: K3 + K4 + gather + K1 + K5), median step
  covered_ms            the same call followed by cordahip_tx_cover_device on the same stream
  cover_in_step_ms      the cover kernel's own device time inside those covered steps (its event
                        pair, cordahip_last_kernel_ms), and cover_share = cover_in_step_ms / baseline_ms
  cover_ms              the cover kernel alone, launched back to back over the statuses the
                        signed-tx call left: its arrays are then warm in the 256 MB Infinity Cache
  cover_shuffled_ms     the same with the key table in random order (a lane's table key is then
                        nowhere near its neighbours': scattered 32-byte reads)
  cover_2of3_ms         the kernel alone on a variant corpus: every required key a 2-of-3 tree
                        (first signer, second signer or a stranger, a stranger): 4 tokens, 3 table
                        keys and the HBM stack per transaction
  bytes_per_tx, gbytes_per_s
                        the bytes a lane needs (offsets, token, table key, its signatures' keys,
                        the statuses it reads and writes) over cover_in_step_ms and over cover_ms;
                        the latter is served largely by the Infinity Cache, so it is not an HBM rate
  clock                 shader clock sampled beside one extra untimed covered step
  mismatches            device tx_status / req_status / first_missing against cordahip_cover_eval_host
                        over the whole corpus (both corpora); must be 0
  host                  cordahip_cover_eval_host on ONE thread over the same corpus (tx/s), and the
                        Python rule of corda_amd/resolve.py over a sample: a floor for an interpreter,
                        NOT a JVM number (nobody has measured the JVM's set build + tree walk)
A run without a GPU fails; nothing falls back.
  python tools/cover_bench.py [--txs 1250000] [--steps 20] [--warmup 3] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12  # MI355X HBM3E peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txs", type=int, default=10_000_000 // 8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--python-sample", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("cover_bench.py: no GPU", file=sys.stderr)
        return 2
    import bench
    from corda_amd import _lib
    from corda_amd import cover as C
    from corda_amd import resolve as R
    from corda_amd.engine import Engine

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    ED = _lib.EDDSA_ED25519_SHA512
    res = {"workload": "tx_cover_device after signed_tx_verify_ed25519_device (c4 corpus in HBM)", "steps": a.steps,
           "warmup": a.warmup}
    with Engine(1) as eng:
        w = bench.C4(eng, dev, stream, 0, bench.parse_args(["--workload", "c4", "--c4-txs", str(a.txs)]))
        ntx, ns = w.ntx, w.ns
        res.update({"txs": ntx, "sigs": ns})
        so = w.tx_sig_off.cpu().numpy().astype(np.uint64)
        keys = w.keys.cpu().numpy()
        nsig = np.diff(so).astype(np.int64)
        first = so[:-1].astype(np.int64)
        rng = np.random.default_rng(0xC07E4)
        ar = np.arange(ntx + 1, dtype=np.uint64)

        def toks(nchild, weight, thr, key):
            t = np.zeros(len(key), _lib.COVER_TOK_DTYPE)
            t["nchild"], t["weight"], t["threshold"], t["key"] = nchild, weight, thr, key
            return t

        # c4: one required key per transaction, a single leaf = the first signer's key
        c4 = C.CoverArrays.from_arrays(ar, ar, toks(0, 1, 0, np.arange(ntx)), np.zeros(ntx, np.uint8),
                                       np.full(ntx, ED, np.uint8), keys[first], ar * 32)
        perm = rng.permutation(ntx)  # table row perm[t] holds transaction t's key
        shuffled_keys = np.empty((ntx, 32), np.uint8)
        shuffled_keys[perm] = keys[first]
        c4s = C.CoverArrays.from_arrays(ar, ar, toks(0, 1, 0, perm), np.zeros(ntx, np.uint8),
                                        np.full(ntx, ED, np.uint8), shuffled_keys, ar * 32)
        # 2-of-3 trees: table = the signature keys, then one stranger per transaction
        strangers = rng.integers(0, 256, (ntx, 32), dtype=np.uint8)
        t_idx = np.arange(ntx, dtype=np.int64)
        leaf_b = np.where(nsig >= 2, first + 1, ns + t_idx)
        leaf_c = np.where(nsig >= 3, first + 2, ns + (t_idx + 1) % ntx)
        tk = np.zeros((ntx, 4), _lib.COVER_TOK_DTYPE)
        tk[:, 0], tk[:, 1], tk[:, 2] = (toks(0, 1, 0, k) for k in (first, leaf_b, leaf_c))
        tk[:, 3] = toks(3, 1, 2, np.zeros(ntx))
        nck = ns + ntx
        c23 = C.CoverArrays.from_arrays(ar, ar * 4, tk.reshape(-1), np.zeros(ntx, np.uint8),
                                        np.full(nck, ED, np.uint8), np.concatenate([keys, strangers]),
                                        np.arange(nck + 1, dtype=np.uint64) * 32)
        dcov = {name: cov.to_device() for name, cov in (("c4", c4), ("c4s", c4s), ("c23", c23))}
        torch.cuda.synchronize(dev)

        def cover(name):
            eng.tx_cover_device(ntx, w.tx_status, w.tx_sig_off, w.keys, dcov[name][0], stream=stream)

        def covered():
            w.step()
            cover("c4")

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(a.warmup):
            w.step()
            covered()
        stream.synchronize()
        base, cov_ms, piped = [], [], []
        for _ in range(a.steps):  # alternating: both legs see the same machine
            base.append(timed(w.step))
            cov_ms.append(timed(covered))
            piped.append(eng.last_kernel_ms())  # this thread's last *_device call: the cover kernel of that step
        # the kernel alone, over the statuses the signed-tx call leaves (restored before every launch)
        w.step()
        stream.synchronize()
        after_verify = w.tx_status.clone()
        host_status = after_verify.cpu().numpy()
        alone, mism = {}, {}
        sch = np.full(ns, ED, np.uint8)
        ko = np.arange(ns + 1, dtype=np.uint64) * 32
        host_s = {}
        for name, cov in (("c4", c4), ("c4s", c4s), ("c23", c23)):
            ms = []
            for i in range(a.warmup + a.steps):
                with torch.cuda.stream(stream):
                    w.tx_status.copy_(after_verify)
                cover(name)
                stream.synchronize()
                if i >= a.warmup:
                    ms.append(eng.last_kernel_ms())
            alone[name] = ms
            t0 = time.perf_counter()
            want_st, want_req, want_first = C.cover_eval_host_arrays(cov, host_status, so, sch, keys.reshape(-1), ko)
            host_s[name] = time.perf_counter() - t0
            got_req, got_first = cov.from_device(dcov[name][1])
            mism[name] = (int((w.tx_status.cpu().numpy() != want_st).sum()) + int((got_req != want_req).sum())
                          + int((got_first != want_first).sum()))
            res["outcomes_" + name] = {str(k): int(v) for k, v in zip(*np.unique(want_st, return_counts=True))}
        b, c = float(np.median(base)), float(np.median(cov_ms))
        k4, k4s, k23 = (float(np.median(alone[n])) for n in ("c4", "c4s", "c23"))
        kp = float(np.median(piped))
        # per transaction: 2 + 2 + 2 offsets (8 B), a 16-B token, the flag, 2 ckey_off, the scheme byte, the 32-B
        # table key, the status read and written, req_status, first_missing, and its signatures' 32-B keys
        bytes_tx = 6 * 8 + 16 + 1 + 2 * 8 + 1 + 32 + 2 + 1 + 8 + 32.0 * ns / ntx
        res.update({"baseline_ms": b, "baseline_ms_min": min(base), "baseline_ms_max": max(base),
                    "covered_ms": c, "covered_ms_min": min(cov_ms), "covered_ms_max": max(cov_ms),
                    "covered_minus_baseline_ms": c - b,
                    "cover_in_step_ms": kp, "cover_in_step_ms_min": min(piped), "cover_in_step_ms_max": max(piped),
                    "cover_share": kp / b,
                    "cover_ms": k4, "cover_ms_min": min(alone["c4"]), "cover_ms_max": max(alone["c4"]),
                    "cover_shuffled_ms": k4s, "cover_2of3_ms": k23,
                    "cover_2of3_share": k23 / b, "txs_per_s_cover": ntx / (kp * 1e-3),
                    "bytes_per_tx": bytes_tx, "gbytes_per_s_in_step": ntx * bytes_tx / (kp * 1e-3) / 1e9,
                    "gbytes_per_s_back_to_back": ntx * bytes_tx / (k4 * 1e-3) / 1e9,
                    "hbm_peak_gbytes_per_s": HBM_BYTES_PER_S / 1e9,
                    "bandwidth_note": "needed bytes over kernel time; back to back the arrays sit in the 256 MB "
                                      "Infinity Cache, so that figure is not an HBM rate",
                    "mismatches": mism})
        res["clock"] = bench._clock_under_load(0, covered, stream.synchronize, c)
        # the host side: the same core on one thread, and the Python rule
        n = min(a.python_sample, ntx)
        sig_keys = [[keys[s].tobytes() for s in range(int(so[t]), int(so[t + 1]))] for t in range(n)]
        must = [[keys[first[t]].tobytes()] for t in range(n)]
        t0 = time.perf_counter()
        miss = 0
        for t in range(n):
            ks = set(sig_keys[t])
            miss += sum(1 for k in must[t] if not R.is_fulfilled_by(k, ks))
        py_s = time.perf_counter() - t0
        table23 = np.concatenate([keys, strangers])
        a23, b23, c23k = (table23[x[:n]] for x in (first, leaf_b, leaf_c))
        must23 = [[R.CompositeKey(2, ((a23[t].tobytes(), 1), (b23[t].tobytes(), 1), (c23k[t].tobytes(), 1)))]
                  for t in range(n)]
        t0 = time.perf_counter()
        for t in range(n):
            ks = set(sig_keys[t])
            miss += sum(1 for k in must23[t] if not R.is_fulfilled_by(k, ks))
        py23_s = time.perf_counter() - t0
        res["host"] = {"cover_eval_host_txs_per_s": ntx / host_s["c4"], "cover_eval_host_2of3_txs_per_s": ntx / host_s["c23"],
                       "threads": 1, "python_rule_txs_per_s": n / py_s, "python_rule_2of3_txs_per_s": n / py23_s,
                       "python_sample": n,
                       "note": "the Python figure is a floor for an interpreter (a set build + isFulfilledBy per "
                               "transaction), not a JVM number"}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if not any(mism.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
