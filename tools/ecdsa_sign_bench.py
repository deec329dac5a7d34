"""ECDSA signing with registered keys on one GPU: the keyed signer (K17,
cordahip_ecdsa_sign_keyed_device) against the corpus signer (cordahip_ecdsa_sign_device:
per-lane key derivation, two gathered fixed-base multiplications, two affine conversions,
a synthetic nonce; its code is not K17's) and against the verifiers over the signatures K17
produced -- the generic one (K2, cordahip_ecdsa_verify_device) and, where the run's keys fit
the verification registry (at most 64), the keyed one (K13,
cordahip_ecdsa_verify_keyed_device) -- on the same 32-byte messages resident in HBM, in ONE
process, the legs alternating step by step so that all see the same machine. Device events
around each launch on the workload's stream. Prints ONE JSON line; per run (a curve choice --
secp256k1, P-256, or the two alternating key by key -- and a key count, lane i signing with
key i mod K):
  keyed_ms, corpus_ms, k2_ms, k13_ms   median step of each leg (min / max beside them)
  *_per_s, keyed_over_corpus = corpus_ms / keyed_ms
  unverified      lanes whose status is not OK, plus lanes K2 (and K13) does not accept; must be 0
  clock           shader clock sampled beside one extra untimed keyed step
The run fails unless every produced signature verifies. A run without a GPU fails; nothing
falls back.
  python tools/ecdsa_sign_bench.py [--lanes 4194304] [--steps 10] [--warmup 2] [--out profiles/NAME.json]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
VKEY_MAX = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--curves", nargs="+", default=["k1", "r1", "alt"], choices=["k1", "r1", "alt"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("ecdsa_sign_bench.py: no GPU", file=sys.stderr)
        return 2
    import bench
    from corda_amd.engine import Engine

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.lanes
    res = {"workload": "ecdsa_sign_keyed_device against ecdsa_sign_device and the verifiers, 32-byte messages in HBM",
           "lanes": n, "steps": a.steps, "warmup": a.warmup, "runs": []}
    bad = 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with Engine(1) as eng:
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x5171)
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        for curves in a.curves:
            for nk in a.keys:
                nk = max(nk, 2) if curves == "alt" else nk
                schemes = [2 if curves == "k1" else 3 if curves == "r1" else 2 + k % 2 for k in range(nk)]
                ds = [hashlib.sha256(b"ecdsa-sign-bench-key-%d" % k).digest() for k in range(nk)]  # < n on both curves
                added = [eng.signer_add_ecdsa(schemes[k], ds[k]) for k in range(nk)]
                assert all(x[1] == 0 for x in added)
                ids = np.array([x[0] for x in added], np.uint32)
                pubs = np.frombuffer(b"".join(x[2] for x in added), np.uint8).reshape(nk, 65)
                lane_key = torch.arange(n, device=dev) % nk
                t_ids = torch.from_numpy(ids.view(np.int32).copy()).to(dev)[lane_key].contiguous()
                t_pubs = torch.from_numpy(pubs.copy()).to(dev)[lane_key].contiguous()
                t_scheme = torch.from_numpy(np.array(schemes, np.uint8)).to(dev)[lane_key].contiguous()
                t_seeds = torch.from_numpy(np.frombuffer(b"".join(ds), np.uint8).reshape(nk, 32).copy()).to(dev)[
                    lane_key].contiguous()
                t_klen = torch.full((n,), 65, dtype=torch.uint8, device=dev)
                ksig = torch.empty((n, 72), dtype=torch.uint8, device=dev)
                klen = torch.empty(n, dtype=torch.uint8, device=dev)
                kst = torch.empty(n, dtype=torch.uint8, device=dev)
                csig = torch.empty((n, 72), dtype=torch.uint8, device=dev)
                clen = torch.empty(n, dtype=torch.uint8, device=dev)
                ckey = torch.empty((n, 65), dtype=torch.uint8, device=dev)
                cklen = torch.empty(n, dtype=torch.uint8, device=dev)
                v2 = torch.empty(n, dtype=torch.uint8, device=dev)
                v13 = torch.zeros(n, dtype=torch.uint8, device=dev)
                with_k13 = nk <= VKEY_MAX
                t_vids = None
                vids = []
                if with_k13:
                    vids = [eng.vkey_add_ecdsa(schemes[k], pubs[k].tobytes()) for k in range(nk)]
                    assert all(x[1] == 0 for x in vids)
                    t_vids = torch.from_numpy(np.array([x[0] for x in vids], np.uint32).view(np.int32).copy()).to(dev)[
                        lane_key].contiguous()
                torch.cuda.synchronize(dev)

                def keyed():
                    eng.ecdsa_sign_keyed_device(t_ids, msgs, ksig, klen, kst, stream=stream)

                def corpus():
                    eng.ecdsa_sign_device(t_scheme, t_seeds, msgs, ckey, cklen, csig, clen, stream=stream)

                def k2():
                    eng.ecdsa_verify_device(t_scheme, t_pubs, t_klen, ksig, klen, msgs, v2, stream=stream)

                def k13():
                    eng.ecdsa_verify_keyed_device(t_vids, ksig, klen, msgs, v13, stream=stream)

                legs = [("keyed", keyed), ("corpus", corpus), ("k2", k2)] + ([("k13", k13)] if with_k13 else [])
                for _ in range(a.warmup):
                    for _, fn in legs:
                        fn()
                stream.synchronize()
                ms = {name: [] for name, _ in legs}
                for _ in range(a.steps):  # alternating: every leg sees the same machine
                    for name, fn in legs:
                        ms[name].append(timed(fn))
                unverified = int((kst != 0).sum()) + int((v2 != 0).sum()) + int((v13 != 0).sum())
                bad += unverified
                run = {"curves": curves, "keys": nk, "unverified": unverified}
                for name, _ in legs:
                    m = float(np.median(ms[name]))
                    run.update({name + "_ms": m, name + "_ms_min": min(ms[name]), name + "_ms_max": max(ms[name]),
                                name + "_per_s": n / (m * 1e-3)})
                run["keyed_over_corpus"] = run["corpus_ms"] / run["keyed_ms"]
                run["clock"] = bench._clock_under_load(0, keyed, stream.synchronize, run["keyed_ms"])
                res["runs"].append(run)
                for kid in ids:
                    eng.signer_remove(int(kid))
                for vid, _ in vids:
                    eng.vkey_remove(vid)
    res["unverified"] = bad
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
