#!/usr/bin/env python3
"""K24 measurements, one JSON line on stdout: registered-key routing inside
cordahip_sig_verify_device on K23's gate batch -- 2^20 signatures, 60 % Ed25519, 35 % ECDSA on both
curves, 5 % RSA-2048, 32-byte messages, about one signature in twenty corrupted -- resident in HBM.
The row pool draws on 62 keys in all (38 Ed25519, 10 per curve, 4 RSA-2048): the registry holds 64
ids across the families.

  (a) the reference: the parent commit's library (--ref-lib; default: this library, switches off)
  (b) this library, the device switch off
  (c) routing on, no lane on a registered key (one foreign key live in each family)
  (d) routing on, every other key of each family registered: about half of each family's lanes keyed
  (e) routing on, every key registered: every lane keyed

Each variant has a context of its own (its registry and switches), all five share the input
tensors. Protocol (r19): two uncounted warm runs of each variant, then the variants alternating,
wall time from the call to the end of a stream synchronisation. Every lane of every run is compared
with (a)'s first run. The gate: (a)'s median minus (e)'s must exceed three times the largest
difference between consecutive (a) runs, with 0 differing lanes."""
import argparse
import ctypes
import hashlib
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "oracle"),
          os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

from sig_device_bench import med, mixed_batch  # noqa: E402

N_ED, N_EC, N_RSA = 38, 20, 4


def pool_rows(oracle):
    """(pools, keys): distinct (scheme, key, sig, msg32) rows per family over N_ED + N_EC + N_RSA keys, one
    row in twenty with a flipped bit; keys: per family, what vkey_add_* takes, in key order; and
    one foreign key per family that signs nothing"""
    import bc_ecdsa as ec
    from test_gpu_rsa_route import by_class, load_keys, sign
    rng = random.Random(2030)
    pub, sig = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
    ed, ecd, rsa = [], [], []
    ed_keys, ec_keys = {}, []
    for i in range(2052):
        m = hashlib.sha256(b"bench-ed-%d" % i).digest()
        oracle.oracle_ed25519_sign(hashlib.sha256(b"seed%d" % (i % N_ED)).digest(), m, 32, pub, sig)
        ed_keys[i % N_ED] = pub.raw
        ed.append((4, pub.raw, sig.raw, m))
    for j in range(N_EC + 2):  # the last two: the foreign keys
        sch = 2 + j % 2
        d = rng.randrange(1, ec.CURVES[sch].n)
        pk = ec.keypair(sch, d)
        ec_keys.append((sch, pk))
        for q in range(4 if j < N_EC else 0):
            m = hashlib.sha256(b"bench-ec-%d-%d" % (j, q)).digest()
            rr, ss = ec.sign(sch, d, m, rng.randrange(1, ec.CURVES[sch].n))
            ecd.append((sch, ec.compress(pk) if (j + q) % 3 == 0 else pk, ec.der_encode(rr, ss), m))
    k64 = by_class(load_keys(), 64)
    assert len(k64) > N_RSA
    for j in range(N_RSA):
        for q in range(3):
            m = hashlib.sha256(b"bench-rsa-%d-%d" % (j, q)).digest()
            rsa.append((1, k64[j]["der"], sign(rng, k64[j], m), m))
    oracle.oracle_ed25519_sign(hashlib.sha256(b"foreign").digest(), b"", 0, pub, sig)

    def spoilt(rows):
        out = list(rows)
        for i in range(0, len(rows), 20):
            s, key, g, m = rows[i]
            g = bytearray(g)
            g[len(g) // 2] ^= 4
            out.append((s, key, bytes(g), m))
        return out
    keys = dict(ed=[ed_keys[i] for i in range(N_ED)], ec=ec_keys[:N_EC], rsa=[k["der"] for k in k64[:N_RSA]],
                foreign=dict(ed=[pub.raw], ec=ec_keys[N_EC:], rsa=[k64[N_RSA]["der"]]))
    return (spoilt(ed), spoilt(ecd), spoilt(rsa)), keys


class Ref:
    """the reference library's cordahip_sig_verify_device on a context of its own"""

    def __init__(self, path):
        self.so = ctypes.CDLL(path)
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
        self.so.cordahip_init.argtypes = [u32, ctypes.POINTER(vp)]
        self.so.cordahip_shutdown.argtypes = [vp]
        self.so.cordahip_sig_verify_device.argtypes = [vp, i32, vp, vp, vp, u64, vp, vp, u64, vp, u32, vp, u64, u64,
                                                       u32, vp, vp, vp]
        self.ctx = vp()
        assert self.so.cordahip_init(1, ctypes.byref(self.ctx)) == 0

    def call(self, d, msgs, status, verdict, s, flags):
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        rc = self.so.cordahip_sig_verify_device(self.ctx, 0, p(d["scheme"]), p(d["key"]), p(d["key_off"]),
                                                d["key"].numel(), p(d["sig"]), p(d["sig_off"]), d["sig"].numel(),
                                                p(msgs), 32, None, msgs.shape[0], d["scheme"].numel(), flags,
                                                p(status), p(verdict), ctypes.c_void_p(s.cuda_stream))
        assert rc == 0, rc

    def close(self):
        self.so.cordahip_shutdown(self.ctx)


def register(e, keys, which):
    """which(i) -> bool over each family's keys; returns the number registered"""
    n = 0
    for i, k in enumerate(keys["ed"]):
        if which(i):
            assert e.vkey_add_ed25519(k)[1] == 0
            n += 1
    for i, (sch, pk) in enumerate(keys["ec"]):
        if which(i // 2):  # the curves alternate in key order
            assert e.vkey_add_ecdsa(sch, pk)[1] == 0
            n += 1
    for i, der in enumerate(keys["rsa"]):
        if which(i):
            assert e.vkey_add_rsa(der)[1] == 0
            n += 1
    return n


def route_on(e):
    e.vkey_set_routing(True)
    e.vkey_set_routing_ecdsa(True)
    e.vkey_set_routing_rsa(True)
    e.vkey_set_routing_device(True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes-log2", type=int, default=20)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--ref-lib", default=None, help="the parent commit's libcordahip.so (default: this library)")
    a = ap.parse_args()
    import torch
    from conftest import load_oracle
    from corda_amd import _lib
    from corda_amd.engine import Engine
    dev = torch.device("cuda:0")
    pools, keys = pool_rows(load_oracle())
    n = 1 << a.lanes_log2
    b = mixed_batch(pools, n)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    d = {k: up(b[k]) for k in ("scheme", "key", "key_off", "sig", "sig_off")}
    msgs = up(b["msg"].reshape(n, 32))
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    verdict = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream(dev)
    ref = Ref(a.ref_lib or _lib.LIB_PATH)
    engines = {v: Engine(1) for v in "bcde"}
    registered = dict(b=0,
                      c=register(engines["c"], keys["foreign"], lambda i: True),
                      d=register(engines["d"], keys, lambda i: i % 2 == 0),
                      e=register(engines["e"], keys, lambda i: True))
    for v in "cde":
        route_on(engines[v])

    def call(v):
        if v == "a":
            ref.call(d, msgs, status, verdict, s, _lib.FLAG_RSA_ON_DEVICE)
        else:
            engines[v].sig_verify_device(d["scheme"], d["key"], d["key_off"], d["sig"], d["sig_off"], msgs, status,
                                         verdict, rsa_on_device=True, stream=s)

    def run(v):
        status.fill_(0xEE)
        torch.cuda.synchronize()
        t = time.perf_counter()
        call(v)
        s.synchronize()
        return (time.perf_counter() - t) * 1e3, status.cpu().numpy()

    order = "abcde"
    stats0 = {v: [engines[v].vkey_route_stats(), engines[v].vkey_route_stats_ecdsa(), engines[v].vkey_route_stats_rsa()]
              for v in "bcde"}
    for v in order:
        for _ in range(2):
            run(v)
    times = {v: [] for v in order}
    differing = {v: 0 for v in order}
    want = None
    for _ in range(a.runs):
        for v in order:
            t, st = run(v)
            want = st if want is None else want
            times[v].append(t)
            differing[v] += int((st != want).sum())
    out = dict(tool="sig_device_route_bench", ref_lib="parent commit" if a.ref_lib else "this library", runs=a.runs,
               lanes=n, shares=dict(zip(("ed25519", "ecdsa", "rsa2048"), (int(x) for x in b["shares"]))),
               keys_in_pool=dict(ed25519=N_ED, ecdsa=N_EC, rsa2048=N_RSA), keys_registered=registered,
               status_histogram={int(k): int(c) for k, c in zip(*np.unique(want, return_counts=True))})
    labels = dict(a="a_reference", b="b_device_switch_off", c="c_routed_no_lane_keyed", d="d_routed_half_keyed",
                  e="e_routed_all_keyed")
    for v in order:
        out[labels[v]] = dict(med(times[v]), differing_lanes=differing[v])
    for v in "cde":  # the share of each family's rows that matched, over the 2 + runs calls
        e = engines[v]
        now = [e.vkey_route_stats(), e.vkey_route_stats_ecdsa(), e.vkey_route_stats_rsa()]
        out[labels[v]]["keyed_share"] = {
            f: round((x[0] - y[0]) / max(1, x[0] - y[0] + x[1] - y[1]), 4)
            for f, x, y in zip(("ed25519", "ecdsa", "rsa2048"), now, stats0[v])}
    ma = out["a_reference"]
    bar = 3 * ma["max_step_ms"]
    for v in "bcde":
        out[labels[v]]["minus_a_ms"] = out[labels[v]]["median_ms"] - ma["median_ms"]
        out[labels[v]]["beyond_bar"] = bool(abs(out[labels[v]]["minus_a_ms"]) > bar)
    total = sum(differing.values())
    out["bar_ms"] = bar
    out["differing_lanes"] = total
    out["gate_met"] = bool(total == 0 and ma["median_ms"] - out["e_routed_all_keyed"]["median_ms"] > bar)
    try:  # the shader clock this box holds under (b), one extra untimed run
        import bench
        out["clock"] = bench._clock_under_load(0, lambda: call("b"), s.synchronize,
                                               out["b_device_switch_off"]["median_ms"])
    except Exception as ex:  # the figures stand without it
        out["clock"] = {"error": repr(ex)}
    for e in engines.values():
        e.close()
    ref.close()
    print(json.dumps(out))
    return 0 if out["gate_met"] else 1


if __name__ == "__main__":
    sys.exit(main())
