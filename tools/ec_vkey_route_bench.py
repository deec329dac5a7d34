"""Routing of registered-key ECDSA lanes (K15, cordahip_vkey_set_routing_ecdsa) on one GPU: the
same call with routing off and on, on the same data, in ONE process, the legs alternating step by
step so that both see the same machine. Prints ONE JSON line.

  dense: cordahip_ecdsa_verify_device over --lanes signatures of 32-byte messages, 1 % with a
    flipped signature bit, device events around each call on the workload's stream. Per curve
    (scheme 2, 3) a fraction f of the lanes (interleaved: lane i is registered when i mod 4 < 4 f)
    carry one of K registered keys (lane i on key i mod K), the others a key of their own. Per
    (scheme, f, K): off_ms / on_ms medians (min, max beside them), ratio = off_ms / on_ms,
    differing_lanes (statuses and verdict words; must be 0), keyed / generic lanes per step from
    cordahip_vkey_route_stats_ecdsa, the shader clock under the routed leg. f = 0: keys registered,
    no lane matches -- the cost of the gather, route and scatter passes and of the indexed generic
    engine. model_ratio: (1 - f) on_ms(f = 0) + f on_ms(f = 1) against off_ms, from this run's own
    f = 0 and f = 1 legs.
  mixed: both curves alternating lane by lane, every lane on a registered key (f = 1, K keys per
    curve): the case in which cordahip_ecdsa_verify_keyed runs both curves' instances over every wave.
  tx: cordahip_tx_submit + cordahip_wait (host CSR arrays, PCIe included, host clock) over --txs
    C4-shaped transactions with two signatures each, an ECDSA notary's (P-256) and a fresh
    secp256k1 key's; 0.5 % of the signatures corrupted. f = 0.5: the notary key registered;
    f = 0: another key registered.
  --ab A.so A2.so B.so: the routing-off path alone. The dense call through three copies of the
    library loaded side by side (A and A2 the same build, e.g. the parent commit's, B this
    one's), alternating step by step: ab_ms medians and b_vs_a against a2_vs_a, the spread of a
    build against itself.
A run without a GPU fails; nothing falls back.
  python tools/ec_vkey_route_bench.py [--lanes 4194304] [--txs 1048576] [--steps 20] [--warmup 3]
      [--out profiles/NAME.json] [--ab A.so A2.so B.so]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

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
        print("ec_vkey_route_bench.py: no GPU", file=sys.stderr)
        return 2
    import bench
    from corda_amd import _lib
    from corda_amd.engine import Engine

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = a.lanes
    res = {"lanes": n, "txs": a.txs, "steps": a.steps, "warmup": a.warmup, "dense": [], "mixed": [], "tx": []}
    bad = 0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def host_timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def seeds_for(registered, reg_seeds, gen):
        """per-lane signing seeds: the registered lanes take reg_seeds[i mod K], the others their own"""
        m = registered.numel()
        s = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device=dev, generator=gen)
        k = (torch.arange(m, device=dev) // 2) % reg_seeds.shape[0]  # i // 2: lanes of one curve when curves alternate
        s[registered] = reg_seeds[k[registered]]
        return s

    def off_on(eng, call, outs_off, outs_on, lanes_per_step, clock=timed):
        """alternating legs; returns the run's figures"""
        def leg(on, outs):
            eng.vkey_set_routing_ecdsa(on)
            call(*outs)
        for _ in range(a.warmup):
            leg(False, outs_off)
            leg(True, outs_on)
        stream.synchronize()
        before = eng.vkey_route_stats_ecdsa()
        t_off, t_on = [], []
        for _ in range(a.steps):
            t_off.append(clock(lambda: leg(False, outs_off)))
            t_on.append(clock(lambda: leg(True, outs_on)))
        after = eng.vkey_route_stats_ecdsa()
        eng.vkey_set_routing_ecdsa(False)
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

    def sign(eng, scheme, seeds, msgs):
        m = scheme.numel()
        keys = torch.zeros((m, 65), dtype=torch.uint8, device=dev)
        sigs = torch.zeros((m, 72), dtype=torch.uint8, device=dev)
        kl, sl = (torch.zeros(m, dtype=torch.uint8, device=dev) for _ in range(2))
        eng.ecdsa_sign_device(scheme, seeds, msgs, keys, kl, sigs, sl, stream=stream)
        stream.synchronize()
        return keys, kl, sigs, sl

    def register(eng, schemes, reg_seeds):
        """the keys d = SHA-256(seed) mod n of the given (scheme, seed) pairs; returns the ids"""
        sc = torch.tensor(schemes, dtype=torch.uint8, device=dev)
        keys, _, _, _ = sign(eng, sc, reg_seeds, torch.zeros((len(schemes), 32), dtype=torch.uint8, device=dev))
        ids = []
        for s, k in zip(schemes, keys.cpu().numpy()):
            kid, st = eng.vkey_add_ecdsa(s, k.tobytes())
            assert st == 0
            ids.append(kid)
        return ids

    with Engine(1) as eng:
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x7E16)
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        words = (n + 63) // 64
        outs = [[torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(words, dtype=torch.int64, device=dev)]
                for _ in range(2)]

        def dense_leg(scheme, registered, reg_seeds, what):
            nonlocal bad
            with torch.cuda.stream(stream):
                keys, kl, sigs, sl = sign(eng, scheme, seeds_for(registered, reg_seeds, gen), msgs)
                flip = torch.arange(0, n, 100, device=dev)  # 1 % corrupted: a bit of the signature's last 16 bytes
                bit = torch.randint(0, 128, (flip.numel(),), device=dev, generator=gen)
                col = sl[flip].to(torch.int64) - 1 - bit // 8
                sigs[flip, col] ^= torch.bitwise_left_shift(torch.ones_like(bit), bit % 8).to(torch.uint8)
            stream.synchronize()

            def call(st, vd):
                eng.ecdsa_verify_device(scheme, keys, kl, sigs, sl, msgs, st, vd, stream=stream)

            run = dict(what, **off_on(eng, call, outs[0], outs[1], n))
            run["rejected_lanes"] = int((outs[0][0] != 0).sum())
            assert run["keyed_lanes_per_step"] == int(registered.sum()), run
            eng.vkey_set_routing_ecdsa(True)
            run["clock"] = bench._clock_under_load(0, lambda: call(*outs[1]), stream.synchronize, run["on_ms"])
            eng.vkey_set_routing_ecdsa(False)
            bad += run["differing_lanes"]
            print(json.dumps(run), file=sys.stderr, flush=True)
            return run

        def key_seeds(tag, nk):
            return torch.from_numpy(np.frombuffer(b"".join(
                hashlib.sha256(b"ec-vkey-route-bench-%s-%d" % (tag, k)).digest() for k in range(nk)),
                np.uint8).reshape(nk, 32).copy()).to(dev)

        # ---- dense, one curve ----
        for sch in (2, 3):
            scheme = torch.full((n,), sch, dtype=torch.uint8, device=dev)
            for nk in a.keys:
                reg_seeds = key_seeds(b"dense", nk)
                ids = register(eng, [sch] * nk, reg_seeds)
                by_f = {}
                for f in a.fractions:
                    registered = (torch.arange(n, device=dev) % 4) < int(round(4 * f))
                    by_f[f] = dense_leg(scheme, registered, reg_seeds, {"scheme": sch, "f": f, "keys": nk})
                    res["dense"].append(by_f[f])
                if 0.0 in by_f and 1.0 in by_f:
                    for f, run in by_f.items():
                        model_on = (1 - f) * by_f[0.0]["on_ms"] + f * by_f[1.0]["on_ms"]
                        run["model_on_ms"] = model_on
                        run["model_ratio"] = run["off_ms"] / model_on
                for kid in ids:
                    eng.vkey_remove(kid)
        # ---- dense, both curves alternating lane by lane, f = 1 ----
        scheme = (2 + (torch.arange(n, device=dev) & 1)).to(torch.uint8)
        for nk in a.keys:
            reg_seeds = key_seeds(b"mixed", nk)
            ids = register(eng, [2] * nk + [3] * nk, torch.cat([reg_seeds, reg_seeds]))
            registered = torch.ones(n, dtype=torch.bool, device=dev)
            res["mixed"].append(dense_leg(scheme, registered, reg_seeds, {"scheme": "2,3 alternating", "f": 1.0,
                                                                          "keys_per_curve": nk}))
            for kid in ids:
                eng.vkey_remove(kid)
        del msgs, outs
        # ---- host signed-tx ----
        ntx = a.txs
        lens = list(bench.C4_LEAF_LENS)
        nl = len(lens)
        leaf_bytes = torch.randint(0, 256, (ntx * sum(lens),), dtype=torch.uint8, device=dev, generator=gen)
        leaf_off = torch.zeros(ntx * nl + 1, dtype=torch.int64, device=dev)
        leaf_off[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64, device=dev).repeat(ntx), 0)
        tx_leaf_off = torch.arange(ntx + 1, dtype=torch.int64, device=dev) * nl
        ns = 2 * ntx
        # the ids: the Ed25519 device signed-tx call with blank signatures
        d_txid = torch.empty((ntx, 32), dtype=torch.uint8, device=dev)
        eng.signed_tx_verify_ed25519_device(
            leaf_bytes, leaf_off, tx_leaf_off, torch.arange(ntx + 1, dtype=torch.int64, device=dev) * 2,
            torch.zeros((ns, 32), dtype=torch.uint8, device=dev), torch.zeros((ns, 64), dtype=torch.uint8, device=dev),
            d_txid, torch.empty(ntx, dtype=torch.uint8, device=dev), torch.empty(ntx, dtype=torch.int64, device=dev),
            torch.empty(ns, dtype=torch.uint8, device=dev), device=0, stream=stream)
        stream.synchronize()
        notary_seed = key_seeds(b"notary", 1)
        is_notary = (torch.arange(ns, device=dev) % 2) == 0
        scheme = torch.where(is_notary, 3, 2).to(torch.uint8)
        m = d_txid.repeat_interleave(2, dim=0).contiguous()
        s = torch.randint(0, 256, (ns, 32), dtype=torch.uint8, device=dev, generator=gen)
        s[is_notary] = notary_seed[0]
        keys, kl, sigs, sl = sign(eng, scheme, s, m)
        flip = torch.randperm(ns, device=dev, generator=gen)[:max(1, ns // 200)]
        sigs[flip, sl[flip].to(torch.int64) - 2] ^= 4
        stream.synchronize()
        h_keys, h_sigs, h_sl = keys.cpu().numpy(), sigs.cpu().numpy(), sl.cpu().numpy().astype(np.uint64)
        sig_off = np.zeros(ns + 1, np.uint64)
        sig_off[1:] = np.cumsum(h_sl)
        sig_flat = h_sigs[np.arange(72)[None, :] < h_sl[:, None]]  # row-major: each row's first sl bytes
        pin = bench._pinned
        t = [pin(x) for x in (leaf_bytes.cpu().numpy(), leaf_off.cpu().numpy().astype(np.uint64),
                              tx_leaf_off.cpu().numpy().astype(np.uint64), np.arange(ntx + 1, dtype=np.uint64) * 2,
                              scheme.cpu().numpy(), h_keys.reshape(-1), np.arange(ns + 1, dtype=np.uint64) * 65,
                              np.ascontiguousarray(sig_flat), sig_off)]
        p = [x.data_ptr() for x in t]
        houts = [tuple(pin(x) for x in (np.zeros((ntx, 32), np.uint8), np.zeros(ntx, np.uint8), np.zeros(ns, np.uint8),
                                         np.zeros(ntx, np.int64))) for _ in range(2)]

        def tx_call(txid, txst, sst, fb):
            tb = _lib.TxidBatch(ntx, p[0], p[1], p[2], txid.data_ptr(), txst.data_ptr(), t[1].numel() - 1, t[0].numel())
            b = _lib.SignedTxBatch(tb, p[3], p[4], p[5], p[6], p[7], p[8], sst.data_ptr(), fb.data_ptr(), ns,
                                   t[5].numel(), t[7].numel())
            tk = ctypes.c_uint64()
            _lib.check(_lib.lib().cordahip_tx_submit(eng.ctx, ctypes.byref(b), ctypes.byref(tk)), "cordahip_tx_submit")
            _lib.check(_lib.lib().cordahip_wait(eng.ctx, tk.value, -1), "cordahip_wait")

        notary_pub = h_keys[0].tobytes()
        for f, tag in ((0.5, None), (0.0, b"other")):
            kid = eng.vkey_add_ecdsa(3, notary_pub)[0] if tag is None else register(eng, [3], key_seeds(tag, 1))[0]
            run = dict({"f": f, "sigs": ns}, **off_on(eng, tx_call, houts[0], houts[1], ns, clock=host_timed))
            run["rejected_sigs"] = int((houts[0][2] != 0).sum())
            run["rejected_txs"] = int((houts[0][1] != 0).sum())
            assert run["keyed_lanes_per_step"] == (ntx if f else 0), run
            bad += run["differing_lanes"]
            res["tx"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
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
        l.cordahip_ecdsa_verify_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, u32, u64, vp, vp, vp]
        l.cordahip_ecdsa_verify_device.restype = i32
        l.cordahip_ecdsa_sign_device.argtypes = [vp, i32, vp, vp, vp, u32, u64, vp, vp, vp, vp, vp]
        l.cordahip_ecdsa_sign_device.restype = i32
        ctx = vp()
        assert l.cordahip_init(1, ctypes.byref(ctx)) == 0, path
        libs.append((l, ctx))
    n = a.lanes
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x7E16)
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
    seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
    scheme = (2 + (torch.arange(n, device=dev) & 1)).to(torch.uint8)
    keys = torch.zeros((n, 65), dtype=torch.uint8, device=dev)
    sigs = torch.zeros((n, 72), dtype=torch.uint8, device=dev)
    kl, sl = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
    l0, c0 = libs[0]
    assert l0.cordahip_ecdsa_sign_device(c0, 0, scheme.data_ptr(), seeds.data_ptr(), msgs.data_ptr(), 32, n,
                                         keys.data_ptr(), kl.data_ptr(), sigs.data_ptr(), sl.data_ptr(),
                                         stream.cuda_stream) == 0
    stream.synchronize()
    flip = torch.arange(0, n, 100, device=dev)
    sigs[flip, sl[flip].to(torch.int64) - 2] ^= 4
    torch.cuda.synchronize(dev)
    words = (n + 63) // 64
    outs = [(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(words, dtype=torch.int64, device=dev))
            for _ in libs]

    def call(k):
        l, ctx = libs[k]
        rc = l.cordahip_ecdsa_verify_device(ctx, 0, scheme.data_ptr(), keys.data_ptr(), kl.data_ptr(), sigs.data_ptr(),
                                            sl.data_ptr(), msgs.data_ptr(), 32, n, outs[k][0].data_ptr(),
                                            outs[k][1].data_ptr(), stream.cuda_stream)
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
    res = {"workload": "ecdsa_verify_device (curves alternating), routing off, three libraries side by side", "lanes": n,
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
