"""A notary's batch of two-input windowed requests, the parent's path against the typed one,
alternating in one process, each on its own commit log that is emptied again after every round
(cordahip_commit_log_revoke of exactly the rows the round committed, untimed), so every round
commits into an empty log with its stage buffers grown:

  (a) cordahip_filtered_tx_verify over the pre-serialised StateRef / TimeWindow leaves, then
      cordahip_commit_inputs with the verify statuses passed through the host as its gate
      (the JVM's Kryo serialisation of those leaves is NOT timed: in (a)'s favour);
  (b) cordahip_notary_tearoff_commit over the typed rows (K21 + K6 + K16 on the log's device).

Both are host forms, so the figures are wall-clock ms of the C calls (stage copies and waits
included) on prebuilt arrays, per batch of `--ntx` tear-offs: median, min and max of `--steps`
alternating rounds after `--warmup`. `device_ms` is cordahip_last_kernel_ms of
cordahip_notary_tearoff_device (K21 + K6 alone, device-resident rows). The statuses of (a) and
(b) must be identical on every transaction of every timed batch (asserted). One JSON line.

  python tools/notary_tearoff_bench.py --out profiles/r27_notary_tearoff.json
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntx", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from corda_amd import _lib
    from corda_amd._lib import lib
    from corda_amd.engine import Engine

    n = a.ntx
    rng = np.random.default_rng(27)
    refs = np.zeros(2 * n, _lib.STATE_REF_DTYPE)
    refs["txhash"] = rng.integers(0, 256, (2 * n, 32), dtype=np.uint8)
    refs["index"] = rng.integers(0, 8, 2 * n)
    fs = np.full(n, 1500000000, np.int64)
    fn = rng.integers(0, 10**9, n).astype(np.int32)
    us = fs + 30
    un = np.zeros(n, np.int32)
    flags = np.full(n, _lib.TW_PRESENT | 3, np.uint8)
    now, tol = 1500000010 * 10**9, 30 * 10**9

    # the leaves: per transaction two refs, two RAW components, the window (host encoder)
    items = []
    rb = refs.tobytes()
    for t in range(n):
        items += [("state_ref", rb[72 * t:72 * t + 36], 0), ("state_ref", rb[72 * t + 36:72 * t + 72], 0),
                  ("raw", hashlib.sha256(b"out %d" % t).digest(), 0), ("raw", b"cmd", 0),
                  ("time_window", _lib.pack_time_window((int(fs[t]), int(fn[t])), (int(us[t]), 0)), 0)]
    leaves = _lib.kryo_encode(items)
    with Engine(1) as eng:
        ids, st, toks = eng.filtered_tx_build([(leaves[5 * t:5 * t + 5], [True, True, False, False, True])
                                               for t in range(n)])
        assert not st.any()
        flat = [k for tk in toks for k in tk]
        tok = np.array([k[0] for k in flat], np.uint8)
        th = np.frombuffer(b"".join(k[1] or bytes(32) for k in flat), np.uint8).copy()
        ko = np.zeros(n + 1, np.uint64)
        ko[1:] = np.cumsum([len(tk) for tk in toks])
        root = np.ascontiguousarray(ids[:n]).reshape(-1).copy()
        # (a): the revealed leaves, serialised
        shown = [leaves[5 * t + i] for t in range(n) for i in (0, 1, 4)]
        lb = np.frombuffer(b"".join(shown), np.uint8).copy()
        lo = np.zeros(3 * n + 1, np.uint64)
        lo[1:] = np.cumsum([len(x) for x in shown])
        to = np.arange(0, 3 * n + 1, 3, dtype=np.uint64)
        ro = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
        caller = np.ones(n, np.uint32)
        twf = (fs * 10**9 + fn).astype(np.int64)
        twu = (us * 10**9 + un).astype(np.int64)
        p = lambda x: x.ctypes.data  # noqa: E731
        out = {k: (np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(2 * n, np.uint8),
                   np.zeros(2 * n, _lib.CONSUMING_TX_DTYPE)) for k in "ab"}
        va, sa, ca, rsa, rba = out["a"]
        _, sb, cb, rsb, rbb = out["b"]
        fa = _lib.FilteredTxBatch(n, p(lb), p(lo), p(to), p(tok), p(th), p(ko), p(root), p(va), 3 * n, lb.size, tok.size)
        cba = _lib.CommitBatch(n, p(root), p(caller), p(refs), p(ro), 2 * n, p(twf), p(twu), now, tol, p(va), p(sa),
                               p(ca), p(rsa), p(rba))
        nb = _lib.NotaryTearoffBatch(n, p(refs), p(ro), 2 * n, p(flags), p(fs), p(fn), p(us), p(un), p(tok), p(th),
                                     p(ko), tok.size, p(root), p(sb), None)
        log2 = max(10, int(np.ceil(np.log2(2 * n * 8 / 7))) + 1)
        ta, tb = [], []
        la, lbg = eng.commit_log_create(log2), eng.commit_log_create(log2)
        rows = np.zeros(2 * n, _lib.COMMIT_ROW_DTYPE)  # what a round commits: ref i by (root of i // 2, i % 2, caller 1)
        rows["ref"] = refs
        rows["by"]["id"] = np.repeat(root.reshape(n, 32), 2, axis=0)
        rows["by"]["input_index"] = np.arange(2 * n) % 2
        rows["by"]["caller"] = 1
        revoked = np.zeros(2 * n, np.uint8)
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            _lib.check(lib().cordahip_filtered_tx_verify(eng.ctx, ctypes.byref(fa)), "filtered_tx_verify")
            _lib.check(lib().cordahip_commit_inputs(eng.ctx, la, ctypes.byref(cba)), "commit_inputs")
            t1 = time.perf_counter()
            _lib.check(lib().cordahip_notary_tearoff_commit(eng.ctx, lbg, ctypes.byref(nb), p(caller), now, tol, None,
                                                            p(cb), p(rsb), p(rbb)), "notary_tearoff_commit")
            t2 = time.perf_counter()
            for log in (la, lbg):
                removed = ctypes.c_uint64()
                _lib.check(lib().cordahip_commit_log_revoke(eng.ctx, log, p(rows), 2 * n, p(revoked),
                                                            ctypes.byref(removed)), "commit_log_revoke")
                assert removed.value == 2 * n
                assert eng.commit_log_stats(log)[0] == 0  # and the host's bound of the entries is exact again
            assert not va.any() and np.array_equal(sa, sb) and np.array_equal(ca, cb) and np.array_equal(rsa, rsb)
            assert int(ca.sum()) == n
            if step >= a.warmup:
                ta.append((t1 - t0) * 1e3)
                tb.append((t2 - t1) * 1e3)
        eng.commit_log_destroy(la)
        eng.commit_log_destroy(lbg)
        # K21 + K6 alone on device-resident rows
        dev = torch.device("cuda", 0)
        up = lambda x, dt=None: torch.from_numpy(x.view(np.uint8) if dt is None else x.astype(dt)).to(dev)  # noqa: E731
        d = dict(refs=up(refs).reshape(-1, 36), ro=up(ro, np.int64), tok=up(tok), th=up(th).reshape(-1, 32),
                 ko=up(ko, np.int64), root=up(root).reshape(-1, 32), fl=up(flags), fs=up(fs), fn=up(fn), us=up(us), un=up(un))
        dst = torch.zeros(n, dtype=torch.uint8, device=dev)
        dtf = torch.zeros(n, dtype=torch.int64, device=dev)
        dtu = torch.zeros(n, dtype=torch.int64, device=dev)
        dms = []
        for step in range(a.warmup + a.steps):
            eng.notary_tearoff_device(d["refs"], d["ro"], d["tok"], d["th"], d["ko"], d["root"], dst, dtf, dtu,
                                      tw_flags=d["fl"], tw_from_s=d["fs"].view(torch.int64), tw_from_nano=d["fn"].view(torch.int32),
                                      tw_until_s=d["us"].view(torch.int64), tw_until_nano=d["un"].view(torch.int32))
            torch.cuda.synchronize(dev)
            if step >= a.warmup:
                dms.append(eng.last_kernel_ms(0))
        assert not dst.any().item() and dtf.cpu().numpy().tolist() == twf.tolist()

    def fig(x):
        return {"median_ms": round(statistics.median(x), 3), "min_ms": round(min(x), 3), "max_ms": round(max(x), 3)}

    res = {"bench": "notary_tearoff", "ntx": n, "inputs": 2, "windowed": True, "steps": a.steps, "warmup": a.warmup,
           "a_filtered_verify_then_commit_inputs": fig(ta), "b_notary_tearoff_commit": fig(tb),
           "k21_k6_device_ms": fig(dms), "statuses_identical": True,
           "bytes_h2d_typed_rows_per_tx": 72 + 25, "leaf_bytes_per_tx_a": int(lb.size // n)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
