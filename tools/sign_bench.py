"""Ed25519 signing with registered keys on one GPU: the keyed signer (K11,
cordahip_ed25519_sign_keyed_device) against the corpus signer of the parent commit
(cordahip_ed25519_sign_device: per-lane key derivation, two fixed-base multiplications with
doublings) on the same 32-byte messages resident in HBM, in ONE process, the legs alternating
step by step so that both see the same machine. Device events around each launch on the
workload's stream. Prints ONE JSON line; per key count (1 and 1,024 registered keys, lane i
signing with key i mod K):
  keyed_ms, corpus_ms     median step of each signer (min / max beside them)
  keyed_per_s, corpus_per_s, speedup = corpus_ms / keyed_ms
  verify_ms, verify_per_s the same lanes' signatures through cordahip_ed25519_verify_device
                          (K1, the C2 shape) in the same process; keyed_over_verify is the
                          signing rate as a fraction of that verification rate
  mismatches              lanes where the two signers' signatures differ, plus lanes whose
                          status is not OK, plus lanes that do not verify; must be 0
  clock                   shader clock sampled beside one extra untimed keyed step
A run without a GPU fails; nothing falls back.
  python tools/sign_bench.py [--lanes 4194304] [--steps 20] [--warmup 3] [--out profiles/NAME.json]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, nargs="+", default=[1, 1024])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("sign_bench.py: no GPU", file=sys.stderr)
        return 2
    import bench
    from corda_amd.engine import Engine

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.lanes
    res = {"workload": "ed25519_sign_keyed_device against ed25519_sign_device, 32-byte messages in HBM", "lanes": n,
           "steps": a.steps, "warmup": a.warmup, "runs": []}
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
        gen.manual_seed(0x5161)
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        for nk in a.keys:
            seeds = np.frombuffer(b"".join(hashlib.sha256(b"sign-bench-key-%d" % k).digest() for k in range(nk)),
                                  np.uint8).reshape(nk, 32)
            added = [eng.signer_add_ed25519(seeds[k].tobytes()) for k in range(nk)]
            ids = np.array([x[0] for x in added], np.uint32)
            pubs = np.frombuffer(b"".join(x[1] for x in added), np.uint8).reshape(nk, 32)
            lane_key = torch.arange(n, device=dev) % nk
            t_ids = torch.from_numpy(ids.view(np.int32).copy()).to(dev)[lane_key].contiguous()
            t_seeds = torch.from_numpy(seeds.copy()).to(dev)[lane_key].contiguous()
            t_pubs = torch.from_numpy(pubs.copy()).to(dev)[lane_key].contiguous()
            ksig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
            kst = torch.empty(n, dtype=torch.uint8, device=dev)
            csig = torch.empty((n, 64), dtype=torch.uint8, device=dev)
            cpub = torch.empty((n, 32), dtype=torch.uint8, device=dev)
            vst = torch.empty(n, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)

            def keyed():
                eng.ed25519_sign_keyed_device(t_ids, msgs, ksig, kst, stream=stream)

            def corpus():
                eng.ed25519_sign_device(t_seeds, msgs, cpub, csig, stream=stream)

            def verify():
                eng.ed25519_verify_device(t_pubs, ksig, msgs, vst, stream=stream)

            for _ in range(a.warmup):
                keyed()
                corpus()
                verify()
            stream.synchronize()
            km, cm, vm = [], [], []
            for _ in range(a.steps):  # alternating: every leg sees the same machine
                km.append(timed(keyed))
                cm.append(timed(corpus))
                vm.append(timed(verify))
            k, c, v = (float(np.median(x)) for x in (km, cm, vm))
            mism = (int((ksig != csig).any(dim=1).sum()) + int((kst != 0).sum()) + int((vst != 0).sum())
                    + int((cpub != t_pubs).any(dim=1).sum()))
            bad += mism
            run = {"keys": nk, "keyed_ms": k, "keyed_ms_min": min(km), "keyed_ms_max": max(km),
                   "corpus_ms": c, "corpus_ms_min": min(cm), "corpus_ms_max": max(cm),
                   "verify_ms": v, "verify_ms_min": min(vm), "verify_ms_max": max(vm),
                   "keyed_per_s": n / (k * 1e-3), "corpus_per_s": n / (c * 1e-3), "verify_per_s": n / (v * 1e-3),
                   "speedup": c / k, "keyed_over_verify": v / k, "mismatches": mism}
            run["clock"] = bench._clock_under_load(0, keyed, stream.synchronize, k)
            res["runs"].append(run)
            for kid in ids:
                eng.signer_remove(int(kid))
    res["mismatches"] = bad
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
