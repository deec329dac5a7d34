"""Routing of registered-key Ed25519 lanes (K14, cordahip_vkey_set_routing) on one GPU: the same
call with routing off and on, on the same data resident in HBM, in ONE process, the legs
alternating step by step so that both see the same machine. Device events around each call on
the workload's stream. Prints ONE JSON line.

  dense: cordahip_ed25519_verify_device over --lanes signatures of 32-byte messages, 1 % with a
    flipped signature bit. A fraction f of the lanes (interleaved: lane i is registered when
    i mod 4 < 4 f) carry one of K registered keys (lane i on key i mod K), the others a key of
    their own. Per (f, K): off_ms / on_ms medians (min, max beside them), ratio = off_ms / on_ms,
    differing_lanes (statuses and verdict words; must be 0), keyed / generic lanes per step from
    cordahip_vkey_route_stats. f = 0: keys registered, no lane matches -- the cost of the route
    and partition pass and of the indexed generic engine. model_ratio: (1 - f) on_ms(f = 0) +
    f on_ms(f = 1) against off_ms, from this run's own f = 0 and f = 1 legs.
  tx: cordahip_signed_tx_verify_ed25519_device over --txs C4-shaped transactions (5 leaves of the
    C4 lengths) with two signatures each, the notary's and a fresh key's; 0.5 % of the signatures
    corrupted. f = 0.5: the notary key registered; f = 0: another key registered.
  --ab A.so A2.so B.so: the routing-off path alone. The dense call through three copies of the
    library loaded side by side (A and A2 the same build, e.g. the parent commit's, B this
    one's), alternating step by step: ab_ms medians and b_vs_a against a2_vs_a, the spread of a
    build against itself.
A run without a GPU fails; nothing falls back.
  python tools/vkey_route_bench.py [--lanes 4194304] [--txs 1048576] [--steps 20] [--warmup 3]
      [--out profiles/NAME.json] [--ab A.so A2.so B.so]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=1 << 22)
    ap.add_argument("--txs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.0, 0.25, 0.5, 1.0])
    ap.add_argument("--keys", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--ab", nargs=3, default=None, metavar=("A.so", "A2.so", "B.so"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("vkey_route_bench.py: no GPU", file=sys.stderr)
        return 2
    import bench
    from corda_amd.engine import Engine

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.lanes
    res = {"lanes": n, "txs": a.txs, "steps": a.steps, "warmup": a.warmup, "dense": [], "tx": []}
    bad = 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def seeds_for(registered, reg_seeds, gen):
        """per-lane signing seeds: the registered lanes take reg_seeds[i mod K], the others their own"""
        m = registered.numel()
        s = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device=dev, generator=gen)
        k = torch.arange(m, device=dev) % reg_seeds.shape[0]
        s[registered] = reg_seeds[k[registered]]
        return s

    def off_on(eng, call, outs_off, outs_on, lanes_per_step):
        """alternating legs; returns the run's figures"""
        def leg(on, outs):
            eng.vkey_set_routing(on)
            call(*outs)
        for _ in range(a.warmup):
            leg(False, outs_off)
            leg(True, outs_on)
        stream.synchronize()
        before = eng.vkey_route_stats()
        t_off, t_on = [], []
        for _ in range(a.steps):
            t_off.append(timed(lambda: leg(False, outs_off)))
            t_on.append(timed(lambda: leg(True, outs_on)))
        after = eng.vkey_route_stats()
        eng.vkey_set_routing(False)
        differ = sum(int((x != y).sum()) for x, y in zip(outs_off, outs_on))
        o, r = stats(t_off), stats(t_on)
        return {"off_ms": o["median"], "off_ms_min": o["min"], "off_ms_max": o["max"],
                "on_ms": r["median"], "on_ms_min": r["min"], "on_ms_max": r["max"],
                "ratio": o["median"] / r["median"], "per_s_off": lanes_per_step / (o["median"] * 1e-3),
                "per_s_on": lanes_per_step / (r["median"] * 1e-3), "differing_lanes": differ,
                "keyed_lanes_per_step": (after[0] - before[0]) // a.steps,
                "generic_lanes_per_step": (after[1] - before[1]) // a.steps}

    if a.ab:
        return ab_main(a, torch, dev, stream, timed)

    with Engine(1) as eng:
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x7E15)
        # ---- dense ----
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        words = (n + 63) // 64
        outs = [[torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(words, dtype=torch.int64, device=dev)]
                for _ in range(2)]
        for nk in a.keys:
            reg_seeds = torch.from_numpy(np.frombuffer(b"".join(
                hashlib.sha256(b"vkey-route-bench-key-%d" % k).digest() for k in range(nk)), np.uint8).reshape(nk, 32).copy()
            ).to(dev)
            reg_pubs = torch.empty((nk, 32), dtype=torch.uint8, device=dev)
            scratch = torch.empty((nk, 64), dtype=torch.uint8, device=dev)
            eng.ed25519_sign_device(reg_seeds, torch.zeros((nk, 32), dtype=torch.uint8, device=dev), reg_pubs, scratch,
                                    stream=stream)
            stream.synchronize()
            ids = []
            for k in reg_pubs.cpu().numpy():
                kid, st = eng.vkey_add_ed25519(k.tobytes())
                assert st == 0
                ids.append(kid)
            by_f = {}
            for f in a.fractions:
                registered = (torch.arange(n, device=dev) % 4) < int(round(4 * f))
                pubs = torch.empty((n, 32), dtype=torch.uint8, device=dev)
                sigs = torch.empty((n, 64), dtype=torch.uint8, device=dev)
                with torch.cuda.stream(stream):
                    eng.ed25519_sign_device(seeds_for(registered, reg_seeds, gen), msgs, pubs, sigs, stream=stream)
                    flip = torch.arange(0, n, 100, device=dev)  # 1 % corrupted
                    bit = torch.randint(0, 512, (flip.numel(),), device=dev, generator=gen)
                    sigs[flip, bit // 8] ^= torch.bitwise_left_shift(torch.ones_like(bit), bit % 8).to(torch.uint8)
                stream.synchronize()

                def call(st, vd):
                    eng.ed25519_verify_device(pubs, sigs, msgs, st, vd, stream=stream)

                run = dict({"f": f, "keys": nk}, **off_on(eng, call, outs[0], outs[1], n))
                run["rejected_lanes"] = int((outs[0][0] != 0).sum())
                assert run["keyed_lanes_per_step"] == int(registered.sum()), run
                eng.vkey_set_routing(True)
                run["clock"] = bench._clock_under_load(0, lambda: call(*outs[1]), stream.synchronize, run["on_ms"])
                eng.vkey_set_routing(False)
                bad += run["differing_lanes"]
                by_f[f] = run
                res["dense"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
                del pubs, sigs
            if 0.0 in by_f and 1.0 in by_f:
                for f, run in by_f.items():
                    model_on = (1 - f) * by_f[0.0]["on_ms"] + f * by_f[1.0]["on_ms"]
                    run["model_on_ms"] = model_on
                    run["model_ratio"] = run["off_ms"] / model_on
            for kid in ids:
                eng.vkey_remove(kid)
        del msgs, outs
        # ---- device signed-tx ----
        ntx = a.txs
        lens = list(bench.C4_LEAF_LENS)
        nl = len(lens)
        leaf_bytes = torch.randint(0, 256, (ntx * sum(lens),), dtype=torch.uint8, device=dev, generator=gen)
        leaf_off = torch.zeros(ntx * nl + 1, dtype=torch.int64, device=dev)
        leaf_off[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64, device=dev).repeat(ntx), 0)
        tx_leaf_off = torch.arange(ntx + 1, dtype=torch.int64, device=dev) * nl
        tx_sig_off = torch.arange(ntx + 1, dtype=torch.int64, device=dev) * 2
        ns = 2 * ntx
        keys = torch.zeros((ns, 32), dtype=torch.uint8, device=dev)
        sigs = torch.zeros((ns, 64), dtype=torch.uint8, device=dev)
        outs = [[torch.empty((ntx, 32), dtype=torch.uint8, device=dev), torch.empty(ntx, dtype=torch.uint8, device=dev),
                 torch.empty(ntx, dtype=torch.int64, device=dev), torch.empty(ns, dtype=torch.uint8, device=dev)]
                for _ in range(2)]

        def tx_call(txid, tst, fb, sst):
            eng.signed_tx_verify_ed25519_device(leaf_bytes, leaf_off, tx_leaf_off, tx_sig_off, keys, sigs, txid, tst, fb,
                                                sst, device=0, stream=stream)

        tx_call(*outs[0])  # the ids (signatures still blank)
        stream.synchronize()
        notary_seed = torch.from_numpy(np.frombuffer(hashlib.sha256(b"vkey-route-bench-notary").digest(), np.uint8).copy()
                                       ).to(dev).reshape(1, 32)
        is_notary = (torch.arange(ns, device=dev) % 2) == 0
        m = outs[0][0].repeat_interleave(2, dim=0).contiguous()
        eng.ed25519_sign_device(seeds_for(is_notary, notary_seed, gen), m, keys, sigs, stream=stream)
        stream.synchronize()
        flip = torch.randperm(ns, device=dev, generator=gen)[:max(1, ns // 200)]
        bit = torch.randint(0, 256, (flip.numel(),), device=dev, generator=gen)
        sigs[flip, bit // 8] ^= torch.bitwise_left_shift(torch.ones_like(bit), bit % 8).to(torch.uint8)
        del m
        notary_pub = keys[0].cpu().numpy().tobytes()
        other_pub = hashlib.sha256(b"vkey-route-bench-other").digest()  # a key no lane carries
        while True:  # until the bytes decode; the probe's slot is freed again
            kid, st = eng.vkey_add_ed25519(other_pub)
            if st == 0:
                eng.vkey_remove(kid)
                break
            other_pub = hashlib.sha256(other_pub).digest()
        for f, pub in ((0.5, notary_pub), (0.0, other_pub)):
            kid = eng.vkey_add_ed25519(pub)[0]
            run = dict({"f": f, "sigs": ns}, **off_on(eng, tx_call, outs[0], outs[1], ns))
            run["rejected_sigs"] = int((outs[0][3] != 0).sum())
            run["rejected_txs"] = int((outs[0][1] != 0).sum())
            assert run["keyed_lanes_per_step"] == (ntx if f else 0), run
            bad += run["differing_lanes"]
            res["tx"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
            if kid is not None:
                eng.vkey_remove(kid)
    res["differing_lanes"] = bad
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad == 0 else 1


def ab_main(a, torch, dev, stream, timed):
    """the dense call, routing never touched, through three side-by-side copies of the library"""
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    libs = []
    for path in a.ab:
        l = ctypes.CDLL(os.path.abspath(path))
        l.cordahip_init.argtypes, l.cordahip_init.restype = [u32, ctypes.POINTER(vp)], i32
        l.cordahip_shutdown.argtypes, l.cordahip_shutdown.restype = [vp], None
        l.cordahip_ed25519_verify_device.argtypes = [vp, i32, vp, vp, vp, u32, u64, vp, vp, vp]
        l.cordahip_ed25519_verify_device.restype = i32
        l.cordahip_ed25519_sign_device.argtypes = [vp, i32, vp, vp, u32, u64, vp, vp, vp]
        l.cordahip_ed25519_sign_device.restype = i32
        ctx = vp()
        assert l.cordahip_init(1, ctypes.byref(ctx)) == 0, path
        libs.append((l, ctx))
    n = a.lanes
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x7E15)
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
    seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
    pubs = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    sigs = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    l0, c0 = libs[0]
    assert l0.cordahip_ed25519_sign_device(c0, 0, seeds.data_ptr(), msgs.data_ptr(), 32, n, pubs.data_ptr(),
                                           sigs.data_ptr(), stream.cuda_stream) == 0
    stream.synchronize()
    flip = torch.arange(0, n, 100, device=dev)
    bit = torch.randint(0, 512, (flip.numel(),), device=dev, generator=gen)
    sigs[flip, bit // 8] ^= torch.bitwise_left_shift(torch.ones_like(bit), bit % 8).to(torch.uint8)
    torch.cuda.synchronize(dev)
    words = (n + 63) // 64
    outs = [(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(words, dtype=torch.int64, device=dev))
            for _ in libs]

    def call(k):
        l, ctx = libs[k]
        rc = l.cordahip_ed25519_verify_device(ctx, 0, pubs.data_ptr(), sigs.data_ptr(), msgs.data_ptr(), 32, n,
                                              outs[k][0].data_ptr(), outs[k][1].data_ptr(), stream.cuda_stream)
        assert rc == 0

    for _ in range(a.warmup):
        for k in range(3):
            call(k)
    stream.synchronize()
    ms = [[], [], []]
    for _ in range(a.steps):
        for k in range(3):
            ms[k].append(timed(lambda: call(k)))
    differ = sum(int((outs[0][j] != outs[k][j]).sum()) for k in (1, 2) for j in (0, 1))
    st = [stats(x) for x in ms]
    res = {"workload": "ed25519_verify_device, routing off, three libraries side by side", "lanes": n,
           "steps": a.steps, "warmup": a.warmup, "libs": [os.path.basename(os.path.dirname(os.path.abspath(p))) for p in a.ab],
           "ab_ms": st, "a2_vs_a": st[1]["median"] / st[0]["median"] - 1, "b_vs_a": st[2]["median"] / st[0]["median"] - 1,
           "b_vs_a2": st[2]["median"] / st[1]["median"] - 1, "rejected_lanes": int((outs[0][0] != 0).sum()),
           "differing_lanes": differ}
    for l, ctx in libs:
        l.cordahip_shutdown(ctx)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if differ == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
