#!/usr/bin/env python3
"""K23 measurements, one JSON line on stdout.

  (b) all-Ed25519 cash-issue component batches: the mixed cordahip_signed_txcomp_verify_device of
      this library against cordahip_signed_txcomp_verify_ed25519_device of the reference library
      (--ref-lib: the parent commit's libcordahip.so; default: this library's own call). The
      difference is what classifying and packing costs a batch that did not need it.
  (c) the gate: a mixed batch (60 % Ed25519, 35 % ECDSA on both curves, 5 % RSA-2048; 2^20
      signatures over 32-byte messages, a share of them corrupted) resident in HBM through
      cordahip_sig_verify_device, against the reference library's cordahip_sig_verify on the same
      rows from pinned host memory (CORDAHIP_FLAG_RSA_ON_DEVICE both). The device call's median must
      be lower, and every lane of every run is compared: 0 differing lanes.
  (a) the packer alone has no entry point of its own; (b)'s difference is its cost on Ed25519 lanes.

Protocol (r19): two uncounted warm runs of each variant, then the variants alternating, wall time
from the call to the end of a stream synchronisation (the host call is synchronous). The rows are
drawn from a pool of distinct signatures made once (pure-Python ECDSA and RSA signing is slow)."""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def pool_rows(oracle):
    """distinct (scheme, key, sig, msg32) rows per family, about one in twenty with a flipped bit"""
    import bc_ecdsa as ec
    from test_gpu_rsa_route import by_class, load_keys, sign
    rng = random.Random(2026)
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    ed, ecd, rsa = [], [], []
    for i in range(2048):
        m = hashlib.sha256(b"bench-ed-%d" % i).digest()
        oracle.oracle_ed25519_sign(hashlib.sha256(b"seed%d" % (i % 64)).digest(), m, 32, pub, sig)
        ed.append((4, pub.raw, sig.raw, m))
    for i in range(96):
        sch = 2 + i % 2
        d = rng.randrange(1, ec.CURVES[sch].n)
        m = hashlib.sha256(b"bench-ec-%d" % i).digest()
        rr, ss = ec.sign(sch, d, m, rng.randrange(1, ec.CURVES[sch].n))
        pk = ec.keypair(sch, d)
        ecd.append((sch, ec.compress(pk) if i % 3 == 0 else pk, ec.der_encode(rr, ss), m))
    k = by_class(load_keys(), 64)[0]
    for i in range(12):
        m = hashlib.sha256(b"bench-rsa-%d" % i).digest()
        rsa.append((1, k["der"], sign(rng, k, m), m))

    def spoilt(rows):
        out = list(rows)
        for i in range(0, len(rows), 20):
            s, key, g, m = rows[i]
            g = bytearray(g)
            g[len(g) // 2] ^= 4
            out.append((s, key, bytes(g), m))
        return out
    return spoilt(ed), spoilt(ecd), spoilt(rsa)


def mixed_batch(pools, n, seed=7):
    rng = np.random.default_rng(seed)
    fam = rng.choice(3, size=n, p=[0.60, 0.35, 0.05])
    pick = [rng.integers(0, len(p), size=n) for p in pools]
    rows = [pools[f][pick[f][i]] for i, f in enumerate(fam.tolist())]
    sch = np.fromiter((r[0] for r in rows), np.uint8, n)
    kl = np.fromiter((len(r[1]) for r in rows), np.int64, n)
    sl = np.fromiter((len(r[2]) for r in rows), np.int64, n)
    ko, so = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    ko[1:], so[1:] = np.cumsum(kl), np.cumsum(sl)
    key = np.frombuffer(b"".join(r[1] for r in rows), np.uint8)
    sig = np.frombuffer(b"".join(r[2] for r in rows), np.uint8)
    msg = np.frombuffer(b"".join(r[3] for r in rows), np.uint8)
    return dict(n=n, scheme=sch, key=key, key_off=ko, sig=sig, sig_off=so, msg=msg, shares=np.bincount(fam, minlength=3))


class RefLib:
    """the reference library's host call over pinned memory"""

    def __init__(self, path):
        from corda_amd import _lib
        self._lib = _lib
        self.so = ctypes.CDLL(path)
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        self.so.cordahip_init.argtypes = [ctypes.c_uint32, ctypes.POINTER(vp)]
        self.so.cordahip_alloc_pinned.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
        self.so.cordahip_sig_verify.argtypes = [vp, ctypes.POINTER(_lib.SigBatch)]
        self.so.cordahip_shutdown.argtypes = [vp]
        self.so.cordahip_signed_txcomp_verify_ed25519_device.argtypes = (
            [vp, ctypes.c_int, vp, u64, ctypes.c_uint32, vp, u64, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp, vp])
        self.ctx = vp()
        assert self.so.cordahip_init(1, ctypes.byref(self.ctx)) == 0

    def pinned(self, a):
        p = ctypes.c_void_p()
        assert self.so.cordahip_alloc_pinned(self.ctx, max(a.nbytes, 16), ctypes.byref(p)) == 0
        out = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(max(a.nbytes, 16),))
        out[:a.nbytes] = a.view(np.uint8).reshape(-1)
        return out[:a.nbytes].view(a.dtype), p

    def host_batch(self, b):
        n = b["n"]
        self.arr = {k: self.pinned(np.ascontiguousarray(v)) for k, v in
                    dict(scheme=b["scheme"], key=b["key"], key_off=b["key_off"].astype(np.uint64), sig=b["sig"],
                         sig_off=b["sig_off"].astype(np.uint64), msg=b["msg"],
                         msg_off=(np.arange(n + 1, dtype=np.uint64) * 32), status=np.zeros(n, np.uint8),
                         verdict=np.zeros((n + 63) // 64, np.uint64)).items()}
        a = {k: v[1] for k, v in self.arr.items()}
        L = self._lib
        self.batch = L.SigBatch(n, *(ctypes.cast(a[k], t) for k, t in zip(
            ("scheme", "key", "key_off", "sig", "sig_off", "msg", "msg_off", "status", "verdict"),
            (f[1] for f in L.SigBatch._fields_[1:10]))), L.FLAG_RSA_ON_DEVICE, b["key"].size, b["sig"].size, n * 32)

    def run_host(self):
        t = time.perf_counter()
        rc = self.so.cordahip_sig_verify(self.ctx, ctypes.byref(self.batch))
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return dt * 1e3, self.arr["status"][0].copy()

    def close(self):
        self.so.cordahip_shutdown(self.ctx)


def med(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), runs=len(xs),
                max_step_ms=max([abs(a - b) for a, b in zip(xs, xs[1:])] or [0.0]))


def gate_c(engine, ref, pools, n, runs):
    import torch
    dev = torch.device("cuda:0")
    b = mixed_batch(pools, n)
    ref.host_batch(b)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = {k: up(b[k]) for k in ("scheme", "key", "key_off", "sig", "sig_off")}
    msgs = up(b["msg"].reshape(n, 32))
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    verdict = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)

    def run_dev():
        status.fill_(0xEE)
        torch.cuda.synchronize()
        t = time.perf_counter()
        engine.sig_verify_device(d["scheme"], d["key"], d["key_off"], d["sig"], d["sig_off"], msgs, status, verdict,
                                 rsa_on_device=True, stream=s)
        s.synchronize()
        return (time.perf_counter() - t) * 1e3, status.cpu().numpy()

    for _ in range(2):
        run_dev(), ref.run_host()
    tdev, thost, differing, want = [], [], 0, None
    for _ in range(runs):
        a, sa = run_dev()
        h, sh = ref.run_host()
        tdev.append(a), thost.append(h)
        want = sh if want is None else want
        differing += int((sa != sh).sum()) + int((sh != want).sum())
    hist = {int(k): int(v) for k, v in zip(*np.unique(want, return_counts=True))}
    dv, hv = med(tdev), med(thost)
    return dict(lanes=n, shares=dict(zip(("ed25519", "ecdsa", "rsa2048"), (int(x) for x in b["shares"]))),
                key_bytes=int(b["key"].size), sig_bytes=int(b["sig"].size), status_histogram=hist,
                device_call=dv, host_call_ref=hv, differing_lanes=differing,
                gate_met=bool(dv["median_ms"] < hv["median_ms"] and differing == 0))


def part_b(engine, ref, oracle, ntx, runs):
    import torch
    from corda_amd import _lib
    from corda_amd.corpus import cash_issue_items
    dev = torch.device("cuda:0")
    g = np.random.default_rng(11)
    blob, items, _ = cash_issue_items(g.integers(0, 256, (ntx, 32), dtype=np.uint8),
                                      g.integers(0, 256, (ntx, 32), dtype=np.uint8), bytes(range(32)),
                                      g.integers(1, 10**9, ntx), g.integers(-2**63, 2**63 - 1, ntx))
    it = items.reshape(-1).copy()
    host_it = it.copy()
    host_it["data"] += np.uint64(blob.ctypes.data)
    hb, ho = _lib.kryo_encode_array(host_it)
    leaves = [[hb[int(ho[5 * t + j]):int(ho[5 * t + j + 1])].tobytes() for j in range(5)] for t in range(ntx)]
    ids, _ = engine.tx_ids(leaves)
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    keys, sigs = bytearray(), bytearray()
    for t in range(ntx):
        oracle.oracle_ed25519_sign(hashlib.sha256(b"b%d" % (t % 64)).digest(), ids[t].tobytes(), 32, pub, sig)
        keys += pub.raw
        sigs += sig.raw if t % 100 else bytes(64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_items, d_blob = up(it.view(np.uint8)), up(blob)
    tio = up(np.arange(0, 5 * ntx + 1, 5, dtype=np.int64))
    tso = up(np.arange(ntx + 1, dtype=np.int64))
    k, sg = up(np.frombuffer(bytes(keys), np.uint8).reshape(ntx, 32)), up(np.frombuffer(bytes(sigs), np.uint8).reshape(ntx, 64))
    sch = torch.full((ntx,), 4, dtype=torch.uint8, device=dev)
    ko, so = up(np.arange(ntx + 1, dtype=np.int64) * 32), up(np.arange(ntx + 1, dtype=np.int64) * 64)
    outs = [(torch.zeros((ntx, 32), dtype=torch.uint8, device=dev), torch.zeros(ntx, dtype=torch.uint8, device=dev),
             torch.zeros(ntx, dtype=torch.int64, device=dev), torch.zeros(ntx, dtype=torch.uint8, device=dev))
            for _ in range(2)]
    s = torch.cuda.Stream(dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        s.synchronize()
        return (time.perf_counter() - t) * 1e3

    def mixed():
        engine.signed_txcomp_verify_device(d_items, len(it), d_blob, tio, tso, sch, k.view(-1), ko, sg.view(-1), so,
                                           *outs[0], stream=s)

    def dense():
        o = outs[1]
        rc = ref.so.cordahip_signed_txcomp_verify_ed25519_device(
            ref.ctx, 0, p(d_items), len(it), 1, p(d_blob), d_blob.numel(), p(tio), ntx, p(tso), p(k), p(sg), ntx,
            p(o[0]), p(o[1]), p(o[2]), p(o[3]), ctypes.c_void_p(s.cuda_stream))
        assert rc == 0, rc

    for _ in range(2):
        timed(mixed), timed(dense)
    tm, td = [], []
    for _ in range(runs):
        tm.append(timed(mixed)), td.append(timed(dense))
    same = all(bool((a == b).all()) for a, b in zip(outs[0], outs[1]))
    m, dn = med(tm), med(td)
    return dict(transactions=ntx, signatures=ntx, mixed_call=m, ed25519_only_call_ref=dn,
                difference_ms=m["median_ms"] - dn["median_ms"], outputs_identical=same,
                rejected=int((outs[0][1] != 0).sum().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes-log2", type=int, default=20)
    ap.add_argument("--tx-log2", type=int, default=16)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--ref-lib", default=None, help="the parent commit's libcordahip.so (default: this library)")
    a = ap.parse_args()
    import torch  # noqa: F401  (first: the libraries then bind to the HIP runtime torch has loaded)
    from conftest import load_oracle
    from corda_amd import _lib
    from corda_amd.engine import Engine
    oracle = load_oracle()
    ref = RefLib(a.ref_lib or _lib.LIB_PATH)
    out = dict(tool="sig_device_bench", ref_lib="parent commit" if a.ref_lib else "this library", runs=a.runs,
               a=dict(packer_alone=None, note="no entry point of its own; b.difference_ms is its cost on Ed25519 lanes"))
    with Engine(1) as engine:
        out["b"] = part_b(engine, ref, oracle, 1 << a.tx_log2, a.runs)
        out["c"] = gate_c(engine, ref, pool_rows(oracle), 1 << a.lanes_log2, a.runs)
    ref.close()
    print(json.dumps(out))
    return 0 if out["c"]["gate_met"] and out["b"]["outputs_identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
