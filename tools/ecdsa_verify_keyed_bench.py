"""ECDSA verification against registered keys on one GPU: the keyed verifier (K13,
cordahip_ecdsa_verify_keyed_device) against the generic verifier of the parent commit
(cordahip_ecdsa_verify_device with each lane's key bytes: key decode, per-lane table, batch
inversion, ladder) on the same signatures over 32-byte ids resident in HBM, in ONE process, the
legs alternating step by step so that both see the same machine. 1 % of the lanes are corrupted
(a bit of r, a bit of the last byte of s, the SEQUENCE tag, in turn). Device events around each
launch on the workload's stream. Prints ONE JSON line; per curve (secp256k1, secp256r1, mixed)
and key count K (lane i on key i mod K; mixed: key k on curve 2 + k mod 2):
  keyed_ms, generic_ms    median step of each verifier (min / max beside them)
  keyed_per_s, generic_per_s, speedup = generic_ms / keyed_ms
  differing_lanes         lanes whose statuses differ between the legs; must be 0
  rejected_lanes          lanes either leg rejects; must equal corrupted_lanes (the tool fails otherwise,
                          and also if a signature verifies under neither leg before it is corrupted)
  vkey_add_ms             host time of one cordahip_vkey_add_ecdsa (median over the K adds)
  clock                   shader clock sampled beside one extra untimed keyed step
A run without a GPU fails; nothing falls back.
  python tools/ecdsa_verify_keyed_bench.py [--lanes 4194304] [--keys 1 16 62] [--steps 20] [--warmup 3]
                                           [--out profiles/NAME.json]
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

CURVES = {"secp256k1": [2], "secp256r1": [3], "mixed": [2, 3]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, nargs="+", default=[1, 16, 62])
    ap.add_argument("--curves", nargs="+", default=list(CURVES), choices=list(CURVES))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("ecdsa_verify_keyed_bench.py: no GPU", file=sys.stderr)
        return 2
    import bench
    from corda_amd.engine import Engine

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.lanes
    res = {"workload": "ecdsa_verify_keyed_device against ecdsa_verify_device, 32-byte ids in HBM, 1% corrupted",
           "lanes": n, "steps": a.steps, "warmup": a.warmup, "runs": []}
    bad = wrong_count = 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    with Engine(1) as eng:
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x7E13)
        with torch.cuda.stream(stream):
            msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        stream.synchronize()
        for cname in a.curves:
            mix = CURVES[cname]
            for nk in a.keys:
                if nk < len(mix):
                    continue
                seeds = np.frombuffer(b"".join(hashlib.sha256(b"ecdsa-keyed-bench-key-%d" % k).digest()
                                               for k in range(nk)), np.uint8).reshape(nk, 32)
                key_sch = np.array([mix[k % len(mix)] for k in range(nk)], np.uint8)
                # everything the signer reads or writes is made on the workload's stream: it does not
                # wait for the default stream, and the allocator reuses the previous run's blocks
                with torch.cuda.stream(stream):
                    lane_key = torch.arange(n, device=dev) % nk
                    t_sch = torch.from_numpy(key_sch).to(dev)[lane_key].contiguous()
                    t_seed = torch.from_numpy(seeds.copy()).to(dev)[lane_key].contiguous()
                    keys = torch.empty((n, 65), dtype=torch.uint8, device=dev)
                    kl = torch.empty(n, dtype=torch.uint8, device=dev)
                    sigs = torch.zeros((n, 72), dtype=torch.uint8, device=dev)
                    sl = torch.empty(n, dtype=torch.uint8, device=dev)
                    eng.ecdsa_sign_device(t_sch, t_seed, msgs, keys, kl, sigs, sl, stream=stream)
                    clean = sigs.clone()
                    lanes = torch.arange(0, n, 100, device=dev)  # 1 % corrupted, three kinds in turn
                    kind = (lanes // 100) % 3
                    sigs[lanes[kind == 0], 10] ^= 4  # a bit of r
                    last = lanes[kind == 1]
                    sigs[last, sl[last].long() - 1] ^= 1  # a bit of the last byte of s
                    sigs[lanes[kind == 2], 0] ^= 1  # the SEQUENCE tag
                    corrupted = int(lanes.numel())
                stream.synchronize()
                pubs = keys[:nk].cpu().numpy()
                add_ms, ids = [], []
                for k in range(nk):
                    t0 = time.perf_counter()
                    kid, st = eng.vkey_add_ecdsa(int(key_sch[k]), pubs[k].tobytes())
                    add_ms.append((time.perf_counter() - t0) * 1e3)
                    assert st == 0
                    ids.append(kid)
                t_ids = torch.from_numpy(np.array(ids, np.uint32).view(np.int32).copy()).to(dev)[lane_key].contiguous()
                kst = torch.empty(n, dtype=torch.uint8, device=dev)
                gst = torch.empty(n, dtype=torch.uint8, device=dev)
                kvd = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
                gvd = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
                torch.cuda.synchronize(dev)
                # the signatures as signed verify on every lane, under both verifiers
                eng.ecdsa_verify_keyed_device(t_ids, clean, sl, msgs, kst, None, stream=stream)
                eng.ecdsa_verify_device(t_sch, keys, kl, clean, sl, msgs, gst, None, stream=stream)
                stream.synchronize()
                for leg, st_ in (("keyed", kst), ("generic", gst)):
                    nz = torch.nonzero(st_ != 0).flatten()
                    assert nz.numel() == 0, "%s leg: %d uncorrupted signatures are not OK (%s %d keys), first lanes %s" % (
                        leg, nz.numel(), cname, nk, nz[:8].tolist())
                del clean

                def keyed():
                    eng.ecdsa_verify_keyed_device(t_ids, sigs, sl, msgs, kst, kvd, stream=stream)

                def generic():
                    eng.ecdsa_verify_device(t_sch, keys, kl, sigs, sl, msgs, gst, gvd, stream=stream)

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
                wrong_count += rejected != corrupted  # every corrupted lane rejects, and no other
                run = {"curve": cname, "keys": nk, "keyed_ms": k, "keyed_ms_min": min(km), "keyed_ms_max": max(km),
                       "generic_ms": g, "generic_ms_min": min(gm), "generic_ms_max": max(gm),
                       "keyed_per_s": n / (k * 1e-3), "generic_per_s": n / (g * 1e-3), "speedup": g / k,
                       "differing_lanes": differ, "rejected_lanes": rejected, "corrupted_lanes": corrupted,
                       "vkey_add_ms": float(np.median(add_ms)), "vkey_add_ms_max": max(add_ms)}
                run["clock"] = bench._clock_under_load(0, keyed, stream.synchronize, k)
                res["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
                for kid in ids:
                    eng.vkey_remove(kid)
    res["differing_lanes"] = bad
    res["runs_with_rejected_not_corrupted"] = wrong_count
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad == 0 and wrong_count == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
