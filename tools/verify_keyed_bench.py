"""Ed25519 verification against registered keys on one GPU: the keyed verifier (K12,
cordahip_ed25519_verify_keyed_device) against the generic verifier of the parent commit
(cordahip_ed25519_verify_device with each lane's key bytes: decompression, joint table,
half-size ladder) on the same signatures over 32-byte ids resident in HBM, in ONE process, the
legs alternating step by step so that both see the same machine. 1 % of the lanes carry a
signature-side corruption (a bit flip anywhere in the signature, bit 255 of S set, S replaced
by random bytes). Device events around each launch on the workload's stream. Prints ONE JSON
line; per key count K (lane i on key i mod K):
  keyed_ms, generic_ms    median step of each verifier (min / max beside them)
  keyed_per_s, generic_per_s, speedup = generic_ms / keyed_ms
  differing_lanes         lanes whose statuses differ between the legs; must be 0
  rejected_lanes          lanes either leg rejects (the corrupted ones)
  vkey_add_ms             host time of one cordahip_vkey_add_ed25519 (median over the K adds;
                          vkey_add_first_ms: the context's first, which allocates the tables)
  clock                   shader clock sampled beside one extra untimed keyed step
A run without a GPU fails; nothing falls back.
  python tools/verify_keyed_bench.py [--lanes 4194304] [--steps 20] [--warmup 3] [--out profiles/NAME.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, nargs="+", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("verify_keyed_bench.py: no GPU", file=sys.stderr)
        return 2
    import bench
    from corda_amd import _lib
    from corda_amd.engine import Engine

    key_counts = a.keys or [1, 16, _lib.VKEY_MAX_KEYS]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.lanes
    res = {"workload": "ed25519_verify_keyed_device against ed25519_verify_device, 32-byte ids in HBM, 1% corrupted",
           "lanes": n, "steps": a.steps, "warmup": a.warmup, "runs": []}
    bad = 0
    first_add_ms = None

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with Engine(1) as eng:
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x7E12)
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        for nk in key_counts:
            seeds = [hashlib.sha256(b"verify-keyed-bench-key-%d" % k).digest() for k in range(nk)]
            signers = [eng.signer_add_ed25519(s) for s in seeds]
            pubs = np.frombuffer(b"".join(x[1] for x in signers), np.uint8).reshape(nk, 32)
            add_ms, ids = [], []
            for k in range(nk):
                t0 = time.perf_counter()
                kid, st = eng.vkey_add_ed25519(pubs[k].tobytes())
                add_ms.append((time.perf_counter() - t0) * 1e3)
                assert st == 0
                ids.append(kid)
            if first_add_ms is None:
                first_add_ms = add_ms[0]
                add_ms = add_ms[1:] or add_ms
            lane_key = torch.arange(n, device=dev) % nk
            t_sid = torch.from_numpy(np.array([x[0] for x in signers], np.uint32).view(np.int32).copy()).to(dev)[lane_key]
            t_ids = torch.from_numpy(np.array(ids, np.uint32).view(np.int32).copy()).to(dev)[lane_key].contiguous()
            t_pubs = torch.from_numpy(pubs.copy()).to(dev)[lane_key].contiguous()
            sigs = torch.empty((n, 64), dtype=torch.uint8, device=dev)
            sst = torch.empty(n, dtype=torch.uint8, device=dev)
            with torch.cuda.stream(stream):
                eng.ed25519_sign_keyed_device(t_sid.contiguous(), msgs, sigs, sst, stream=stream)
                # 1 % corrupted, three kinds in turn
                lanes = torch.arange(0, n, 100, device=dev)
                kind = (lanes // 100) % 3
                flip = lanes[kind == 0]
                bit = torch.randint(0, 512, (flip.numel(),), device=dev, generator=gen)
                sigs[flip, bit // 8] ^= torch.bitwise_left_shift(torch.ones_like(bit), bit % 8).to(torch.uint8)
                sigs[lanes[kind == 1], 63] |= 0x80
                rnd = lanes[kind == 2]
                sigs[rnd, 32:] = torch.randint(0, 256, (rnd.numel(), 32), dtype=torch.uint8, device=dev, generator=gen)
            stream.synchronize()
            assert int((sst != 0).sum()) == 0
            for kid, _ in signers:
                eng.signer_remove(kid)
            kst = torch.empty(n, dtype=torch.uint8, device=dev)
            gst = torch.empty(n, dtype=torch.uint8, device=dev)
            kvd = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
            gvd = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
            torch.cuda.synchronize(dev)

            def keyed():
                eng.ed25519_verify_keyed_device(t_ids, sigs, msgs, kst, kvd, stream=stream)

            def generic():
                eng.ed25519_verify_device(t_pubs, sigs, msgs, gst, gvd, stream=stream)

            for _ in range(a.warmup):
                keyed()
                generic()
            stream.synchronize()
            km, gm = [], []
            for _ in range(a.steps):  # alternating: both legs see the same machine
                km.append(timed(keyed))
                gm.append(timed(generic))
            k, g = float(np.median(km)), float(np.median(gm))
            differ = int((kst != gst).sum()) + int((kvd != gvd).sum())
            rejected = int((gst != 0).sum())
            bad += differ
            run = {"keys": nk, "keyed_ms": k, "keyed_ms_min": min(km), "keyed_ms_max": max(km),
                   "generic_ms": g, "generic_ms_min": min(gm), "generic_ms_max": max(gm),
                   "keyed_per_s": n / (k * 1e-3), "generic_per_s": n / (g * 1e-3), "speedup": g / k,
                   "differing_lanes": differ, "rejected_lanes": rejected,
                   "vkey_add_ms": float(np.median(add_ms)), "vkey_add_ms_max": max(add_ms)}
            run["clock"] = bench._clock_under_load(0, keyed, stream.synchronize, k)
            res["runs"].append(run)
            for kid in ids:
                eng.vkey_remove(kid)
    res["vkey_add_first_ms"] = first_add_ms
    res["differing_lanes"] = bad
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
