"""RSA_SHA256 (RSASSA-PSS) throughput of the dense device path on one GPU.

2^18 resident 3072-bit rows (cordahip_rsa_pss_verify_device; a handful of distinct keys,
256 distinct CRT-made signatures tiled over the rows, 1 % of the rows corrupted), timed
with device events over >= 20 steps after warm-up. Prints ONE JSON line:
  verifs_per_s          rows / median step time of the whole verification
  verify_ms             median device time of one step (prep + modexp + check kernels)
  modexp_ms             the modular exponentiation alone (cordahip_rsa_public_op_device over
                        the same moduli, exponents and signatures), its own timed steps
  prep_check_ms         verify_ms - modexp_ms: the prep and PSS check kernels
  limb_macs_per_s, fraction_of_peak
                        32x32-bit multiply-accumulates the algorithm needs (2 W^2 per
                        Montgomery product; products = squarings for R^2, to and from
                        Montgomery form, one per exponent bit below the top, one per set
                        bit below the top) over modexp_ms, against the 39.3 T limb-MAC/s
                        peak DESIGN.md §4 uses
  clock                 shader clock sampled beside one extra untimed step (bench.py's sampler)
  cpu                   16 threads of OpenSSL libcrypto verifying the same rows on this box
                        (through ctypes: the threads share the interpreter between calls, so this
                        is a floor for the CPU, not its best), or the reason it could not run
A run without a GPU fails; nothing falls back.
  python tools/rsa_bench.py [--rows-log2 18] [--steps 20] [--warmup 3] [--out profiles/NAME.json]

--keyed: the registered-key verifier (K18) against the generic one, A/B in one process on one box.
The same resident rows go through cordahip_rsa_pss_verify_device and, their keys registered,
through cordahip_rsa_verify_keyed_device, the two calls alternating step by step on one stream,
timed with device events; every lane's status is compared between the two. Four legs: the
3072-bit rows above (some of their keys are shorter than their class), one 3072-bit key alone, then
the 2048-bit class with a 1024-bit key and with a 2048-bit key. Per leg:
  generic_ms, keyed_ms      median step times (min, max beside them), ratio = generic / keyed
  generic_spread_ms         the largest difference between consecutive generic steps; the bar is
                            generic_ms - keyed_ms > 3 x that (over_bar)
  modexp_generic_ms, modexp_keyed_ms
                            the modular exponentiations alone (the two raw ops), alternating too
  products_generic, products_keyed, model_ratio
                            the product counts of the two schedules and the step ratio they predict
                            when only the modexp share of the generic step shrinks
  differing_lanes           lanes whose statuses differ between the two calls (must be 0)

--routed: routing of registered-key rows (K20, cordahip_vkey_set_routing_rsa) A/B in one process on one
box. The same resident rows go through cordahip_rsa_pss_verify_device with routing off and on, the
two alternating step by step on one stream, timed with device events; every lane's status is compared
between the legs. Legs: one 3072-bit key and one 2048-bit key registered, with f = 0, 0.5 and 1 of the
rows (interleaved) on the registered key and the others on an unregistered key of the same size; at
f = 1 cordahip_rsa_verify_keyed_device is a third alternating leg. Per leg:
  off_ms, on_ms (and keyed_ms)   median step times with min and max
  off_spread_ms                  the largest difference between consecutive off steps; the bar is
                                 off_ms - on_ms > 3 x that (over_bar)
  keyed_rows, generic_rows       cordahip_vkey_route_stats_rsa's movement over one routed step
  differing_lanes                must be 0
and per key model_half_ms = 0.5 on_ms(f = 0) + 0.5 on_ms(f = 1) beside the measured on_ms(f = 0.5).

--ab A.so A2.so B.so: the routing-off path alone. The dense call through three copies of the library
loaded side by side (A and A2 the same build, e.g. the parent commit's, B this one), alternating;
b_vs_a must sit inside a2_vs_a's size.
"""
import argparse
import json
import os
import random
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

PEAK_LIMB_MACS = 39.3e12  # 256 CU x 64 lane-MACs per CU-cycle x 2.4 GHz
W = 96


def products(e):
    """Montgomery products rsa_modexp_kernel<96> runs for a wave of exponent e."""
    sq = (32 * W & -(32 * W)).bit_length() - 1  # squarings from 2^s R to R^2 (32 W = s 2^sq)
    top = e.bit_length() - 1
    return sq + 1 + top + bin(e).count("1") - 1 + 1


def products_at(e, w, keyed):
    """Montgomery products of a wave of exponent e in class w: rsa_modexp_kernel (squarings for R^2, in
    and out of Montgomery form, the chain) or rsa_modexp_keyed_kernel (the chain and the product with K)."""
    chain = e.bit_length() - 1 + bin(e).count("1") - 1
    if keyed:
        return chain + 1
    return (32 * w & -(32 * w)).bit_length() - 1 + 1 + chain + 1


def keyed_leg(torch, eng, a, name, w, keys, rng):
    """one A/B leg: n rows of class w over `keys`, generic and keyed alternating"""
    import bc_rsa_pss as bc
    n = 1 << a.rows_log2
    dist = []
    for i in range(a.distinct):
        k = keys[i % len(keys)]
        m = rng.randbytes(32)
        em = bc.encode_em(m, k["n"].bit_length(), rng.randbytes(32))
        sig = bc.sign_crt(em, k["p"], k["q"], k["d"]).to_bytes((k["n"].bit_length() + 7) // 8, "big")
        dist.append((i % len(keys), sig, m))
    ids = []
    for k in keys:
        kid, st = eng.vkey_add_rsa(bc.encode_key(k["n"], k["e"]))
        assert st == 0, st
        ids.append(kid)
    mod = np.zeros((a.distinct, w), np.uint32)
    exp = np.zeros(a.distinct, np.uint32)
    kid = np.zeros(a.distinct, np.uint32)
    sigs = np.zeros((a.distinct, 4 * w), np.uint8)
    sl = np.zeros(a.distinct, np.uint16)
    msgs = np.zeros((a.distinct, 32), np.uint8)
    words = np.zeros((a.distinct, w), np.uint32)
    for i, (ki, sig, m) in enumerate(dist):
        k = keys[ki]
        mod[i] = np.frombuffer(k["n"].to_bytes(4 * w, "little"), "<u4")
        exp[i] = k["e"]
        kid[i] = ids[ki]
        sigs[i, :len(sig)] = np.frombuffer(sig, np.uint8)
        sl[i] = len(sig)
        msgs[i] = np.frombuffer(m, np.uint8)
        words[i] = np.frombuffer(int.from_bytes(sig, "big").to_bytes(4 * w, "little"), "<u4")
    idx = np.arange(n) % a.distinct
    bad = np.zeros(n, bool)
    bad[rng.sample(range(n), n // 100)] = True
    rows_sig = sigs[idx]
    rows_sig[bad, 100] ^= 0x10  # 1 % corrupted
    dev = torch.device("cuda:0")
    t = lambda x, ty: torch.from_numpy(np.ascontiguousarray(x).view(ty)).to(dev)  # noqa: E731
    tm, te, tw, tk = t(mod[idx], np.int32), t(exp[idx], np.int32), t(words[idx], np.int32), t(kid[idx], np.int32)
    ts, tl, tg = t(rows_sig, np.uint8), t(sl[idx], np.int16), t(msgs[idx], np.uint8)
    st_g = torch.empty(n, dtype=torch.uint8, device=dev)
    st_k = torch.empty(n, dtype=torch.uint8, device=dev)
    verdict = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    out_g = torch.empty((n, w), dtype=torch.int32, device=dev)
    out_k = torch.empty((n, w), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)

    def alternate(fa, fb):
        ms = ([], [])
        for step in range(a.warmup + a.steps):
            for which, fn in enumerate((fa, fb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if step >= a.warmup:
                    ms[which].append(e0.elapsed_time(e1))
        return ms
    gms, kms = alternate(lambda: eng.rsa_pss_verify_device(tm, te, ts, tl, tg, st_g, verdict, stream=stream),
                         lambda: eng.rsa_verify_keyed_device(tk, ts, tl, tg, st_k, verdict, stream=stream))
    sg, sk = st_g.cpu().numpy(), st_k.cpu().numpy()
    differing = int((sg != sk).sum())
    assert int((sg == 0).sum()) == n - int(bad.sum()) and (sg[bad] == 1).all(), "wrong statuses"
    mg, mk = alternate(lambda: eng.rsa_public_op_device(tm, te, tw, out_g, stream=stream),
                       lambda: eng.rsa_public_op_keyed_device(tk, tw, out_k, stream=stream))
    rows_differ = int((out_g != out_k).any(dim=1).sum().item())
    for i in ids:
        eng.vkey_remove(i)
    med = lambda v: float(np.median(v))  # noqa: E731
    spread = max(abs(x - y) for x, y in zip(gms, gms[1:])) if len(gms) > 1 else 0.0
    e = keys[0]["e"]
    pg, pk = products_at(e, w, False), products_at(e, w, True)
    share = med(mg) / med(gms)  # the modexp's share of the generic step, this run
    return {"leg": name, "rows": n, "mod_words": w, "modulus_bits": sorted({k["n"].bit_length() for k in keys}),
            "keys": len(keys), "e": e, "distinct_signatures": a.distinct, "corrupted_rows": int(bad.sum()),
            "generic_ms": med(gms), "generic_ms_min": min(gms), "generic_ms_max": max(gms),
            "keyed_ms": med(kms), "keyed_ms_min": min(kms), "keyed_ms_max": max(kms),
            "generic_spread_ms": spread, "ratio": med(gms) / med(kms),
            "over_bar": bool(med(gms) - med(kms) > 3 * spread),
            "modexp_generic_ms": med(mg), "modexp_keyed_ms": med(mk), "modexp_ratio": med(mg) / med(mk),
            "modexp_share_of_generic": share, "products_generic": pg, "products_keyed": pk,
            "model_ratio": 1.0 / (1.0 - share + share * pk / pg),
            "keyed_verifs_per_s": n / (med(kms) * 1e-3), "generic_verifs_per_s": n / (med(gms) * 1e-3),
            "differing_lanes": differing, "differing_modexp_rows": rows_differ}


def keyed_main(a):
    import torch
    if not torch.cuda.is_available():
        print("rsa_bench.py: no GPU", file=sys.stderr)
        return 2
    from corda_amd.engine import Engine
    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        g = json.load(f)
    fix = [{f: int(k[f], 16) for f in ("n", "e", "d", "p", "q")} for k in g["keys"]
           if "d" in k and int(k["e"], 16) == 65537]
    k3072 = [k for k in fix if 2048 < k["n"].bit_length() <= 3072]
    try:
        import openssl_rsa_pss as ossl
        for _ in range(2):  # the same handful of keys as the plain run: two more from OpenSSL where it loads
            h, k = ossl.keygen(3072)
            ossl.free_key(h)
            k3072.append(k)
    except (OSError, AttributeError, AssertionError):
        pass
    legs = [("3072-bit rows", 96, k3072),
            ("3072-bit class, a 3072-bit key", 96, [k for k in fix if k["n"].bit_length() == 3072][:1]),
            ("2048-bit class, a 1024-bit key", 64, [k for k in fix if k["n"].bit_length() == 1024][:1]),
            ("2048-bit class, a 2048-bit key", 64, [k for k in fix if k["n"].bit_length() == 2048][:1])]
    rng = random.Random(0xBE7C)
    res = {"workload": "rsa_verify_keyed_device against rsa_pss_verify_device, alternating", "steps": a.steps,
           "warmup": a.warmup, "legs": []}
    with Engine(1) as eng:
        for name, w, keys in legs:
            assert keys, name
            res["legs"].append(keyed_leg(torch, eng, a, name, w, keys, rng))
    res["differing_lanes"] = sum(l["differing_lanes"] for l in res["legs"])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["differing_lanes"] == 0 else 1


def fixture_keys():
    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        g = json.load(f)
    return [{f: int(k[f], 16) for f in ("n", "e", "d", "p", "q")} for k in g["keys"]
            if "d" in k and int(k["e"], 16) == 65537]


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


_SIGNED = {}


def dense_rows(torch, a, w, keys, share, rng):
    """n resident rows of class w: `share` of them (interleaved) on keys[0], the others on keys[1];
    a.distinct CRT signatures per key tiled, 1 % of the rows corrupted. Device tensors and the bad mask."""
    import bc_rsa_pss as bc
    n = 1 << a.rows_log2
    per = []
    for k in keys:
        if (k["n"], w) in _SIGNED:  # a key's signatures are made once per run
            per.append(_SIGNED[(k["n"], w)])
            continue
        mod = np.frombuffer(k["n"].to_bytes(4 * w, "little"), "<u4")
        sigs = np.zeros((a.distinct, 4 * w), np.uint8)
        sl = np.zeros(a.distinct, np.uint16)
        msgs = np.zeros((a.distinct, 32), np.uint8)
        for i in range(a.distinct):
            m = rng.randbytes(32)
            em = bc.encode_em(m, k["n"].bit_length(), rng.randbytes(32))
            sig = bc.sign_crt(em, k["p"], k["q"], k["d"]).to_bytes((k["n"].bit_length() + 7) // 8, "big")
            sigs[i, :len(sig)] = np.frombuffer(sig, np.uint8)
            sl[i] = len(sig)
            msgs[i] = np.frombuffer(m, np.uint8)
        _SIGNED[(k["n"], w)] = (mod, sigs, sl, msgs)
        per.append(_SIGNED[(k["n"], w)])
    r = np.arange(n)
    on_first = np.floor((r + 1) * share) > np.floor(r * share)  # interleaved: every 1 / share-th row
    which = np.where(on_first, 0, 1)
    idx = r % a.distinct
    mod = np.stack([per[0][0], per[1][0]])[which]
    exp = np.array([keys[0]["e"], keys[1]["e"]], np.uint32)[which]
    sigs = np.where(on_first[:, None], per[0][1][idx], per[1][1][idx])
    sl = np.where(on_first, per[0][2][idx], per[1][2][idx]).astype(np.uint16)
    msgs = np.where(on_first[:, None], per[0][3][idx], per[1][3][idx])
    bad = np.zeros(n, bool)
    bad[rng.sample(range(n), n // 100)] = True
    sigs[bad, 100] ^= 0x10  # 1 % corrupted
    dev = torch.device("cuda:0")
    t = lambda x, ty: torch.from_numpy(np.ascontiguousarray(x).view(ty)).to(dev)  # noqa: E731
    return (t(mod, np.int32), t(exp, np.int32), t(sigs, np.uint8), t(sl, np.int16), t(msgs, np.uint8)), bad, on_first


def routed_main(a):
    import torch
    if not torch.cuda.is_available():
        print("rsa_bench.py: no GPU", file=sys.stderr)
        return 2
    import bc_rsa_pss as bc
    from corda_amd.engine import Engine
    fix = fixture_keys()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    rng = random.Random(0xBE20)
    n = 1 << a.rows_log2

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    res = {"workload": "rsa_pss_verify_device, RSA routing off and on alternating", "rows": n, "steps": a.steps,
           "warmup": a.warmup, "distinct_signatures_per_key": a.distinct, "legs": [], "models": []}
    with Engine(1) as eng:
        for bits, w in ((3072, 96), (2048, 64)):
            same = [k for k in fix if k["n"].bit_length() == bits]
            other = same[1:2]
            if not other:  # the fixture has one such key: another of the size from OpenSSL, else the nearest
                try:
                    import openssl_rsa_pss as ossl
                    h, k = ossl.keygen(bits)
                    ossl.free_key(h)
                    other = [k]
                except (OSError, AttributeError, AssertionError):
                    other = [k for k in fix if k["n"].bit_length() == bits - 1][:1]
            keys = [same[0], other[0]]
            kid, st = eng.vkey_add_rsa(bc.encode_key(keys[0]["n"], keys[0]["e"]))
            assert st == 0, st
            on_ms = {}
            for share in (0.0, 0.5, 1.0):
                (tm, te, ts, tl, tg), bad, on_first = dense_rows(torch, a, w, keys, share, rng)
                st_off = torch.empty(n, dtype=torch.uint8, device=dev)
                st_on = torch.empty(n, dtype=torch.uint8, device=dev)
                st_k = torch.empty(n, dtype=torch.uint8, device=dev)
                verdict = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
                tk = torch.full((n,), kid, dtype=torch.int64, device=dev).to(torch.int32)

                def leg_off():
                    eng.vkey_set_routing_rsa(False)
                    eng.rsa_pss_verify_device(tm, te, ts, tl, tg, st_off, verdict, stream=stream)

                def leg_on():
                    eng.vkey_set_routing_rsa(True)
                    eng.rsa_pss_verify_device(tm, te, ts, tl, tg, st_on, verdict, stream=stream)

                def leg_keyed():
                    eng.rsa_verify_keyed_device(tk, ts, tl, tg, st_k, verdict, stream=stream)

                fns = [leg_off, leg_on] + ([leg_keyed] if share == 1.0 else [])
                ms = [[] for _ in fns]
                for step in range(a.warmup + a.steps):
                    for q, fn in enumerate(fns):
                        v = timed(fn)
                        if step >= a.warmup:
                            ms[q].append(v)
                before = eng.vkey_route_stats_rsa()
                leg_on()
                stream.synchronize()
                after = eng.vkey_route_stats_rsa()
                eng.vkey_set_routing_rsa(False)
                s_off, s_on = st_off.cpu().numpy(), st_on.cpu().numpy()
                differing = int((s_off != s_on).sum())
                assert int((s_off == 0).sum()) == n - int(bad.sum()) and (s_off[bad] == 1).all(), "wrong statuses"
                if share == 1.0:
                    differing += int((st_k.cpu().numpy() != s_off).sum())
                off, on = stats(ms[0]), stats(ms[1])
                spread = max(abs(x - y) for x, y in zip(ms[0], ms[0][1:])) if len(ms[0]) > 1 else 0.0
                leg = {"modulus_bits": bits, "mod_words": w, "other_key_bits": keys[1]["n"].bit_length(), "f": share,
                       "off_ms": off, "on_ms": on, "off_spread_ms": spread, "ratio": off["median"] / on["median"],
                       "margin_ms": off["median"] - on["median"],
                       "over_bar": bool(off["median"] - on["median"] > 3 * spread),
                       "keyed_rows": after[0] - before[0], "generic_rows": after[1] - before[1],
                       "rows_on_registered_key": int(on_first.sum()), "differing_lanes": differing,
                       "off_verifs_per_s": n / (off["median"] * 1e-3), "on_verifs_per_s": n / (on["median"] * 1e-3)}
                if share == 1.0:
                    kd = stats(ms[2])
                    leg.update({"keyed_ms": kd, "routed_over_id_keyed": on["median"] / kd["median"],
                                "off_over_id_keyed": off["median"] / kd["median"]})
                assert leg["keyed_rows"] == leg["rows_on_registered_key"] and leg["keyed_rows"] + leg["generic_rows"] == n
                on_ms[share] = on["median"]
                res["legs"].append(leg)
            eng.vkey_remove(kid)
            res["models"].append({"modulus_bits": bits, "on_half_ms": on_ms[0.5],
                                  "model_half_ms": 0.5 * on_ms[0.0] + 0.5 * on_ms[1.0]})
    res["differing_lanes"] = sum(l["differing_lanes"] for l in res["legs"])
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["differing_lanes"] == 0 else 1


def ab_main(a):
    """the dense call, routing never touched, through three side-by-side copies of the library"""
    import ctypes

    import torch
    if not torch.cuda.is_available():
        print("rsa_bench.py: no GPU", file=sys.stderr)
        return 2
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    libs = []
    for path in a.ab:
        l = ctypes.CDLL(os.path.abspath(path))
        l.cordahip_init.argtypes, l.cordahip_init.restype = [u32, ctypes.POINTER(vp)], i32
        l.cordahip_shutdown.argtypes, l.cordahip_shutdown.restype = [vp], None
        l.cordahip_rsa_pss_verify_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, u32, u32, u64, vp, vp, vp]
        l.cordahip_rsa_pss_verify_device.restype = i32
        ctx = vp()
        assert l.cordahip_init(1, ctypes.byref(ctx)) == 0, path
        libs.append((l, ctx))
    fix = fixture_keys()
    keys = [k for k in fix if k["n"].bit_length() == 3072][:1] + [k for k in fix if k["n"].bit_length() == 3071][:1]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = 1 << a.rows_log2
    (tm, te, ts, tl, tg), bad, _ = dense_rows(torch, a, 96, keys, 0.5, random.Random(0xBEAB))
    outs = [(torch.empty(n, dtype=torch.uint8, device=dev), torch.empty((n + 63) // 64, dtype=torch.int64, device=dev))
            for _ in libs]

    def call(k):
        l, ctx = libs[k]
        rc = l.cordahip_rsa_pss_verify_device(ctx, 0, tm.data_ptr(), te.data_ptr(), ts.data_ptr(), tl.data_ptr(),
                                              tg.data_ptr(), 32, 96, n, outs[k][0].data_ptr(), outs[k][1].data_ptr(),
                                              stream.cuda_stream)
        assert rc == 0

    ms = [[], [], []]
    for step in range(a.warmup + a.steps):
        for k in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call(k)
            e1.record(stream)
            e1.synchronize()
            if step >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    differ = sum(int((outs[0][j] != outs[k][j]).sum()) for k in (1, 2) for j in (0, 1))
    st = [stats(x) for x in ms]
    res = {"workload": "rsa_pss_verify_device (3072-bit class), routing off, three libraries side by side", "rows": n,
           "steps": a.steps, "warmup": a.warmup,
           "libs": [os.path.basename(os.path.dirname(os.path.abspath(p))) for p in a.ab], "ab_ms": st,
           "a2_vs_a": st[1]["median"] / st[0]["median"] - 1, "b_vs_a": st[2]["median"] / st[0]["median"] - 1,
           "b_vs_a2": st[2]["median"] / st[1]["median"] - 1, "rejected_rows": int((outs[0][0] != 0).sum()),
           "differing_lanes": differ}
    for l, ctx in libs:
        l.cordahip_shutdown(ctx)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if differ == 0 else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=18)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-rows", type=int, default=1 << 14)
    ap.add_argument("--out", default=None)
    ap.add_argument("--keyed", action="store_true", help="A/B of the registered-key verifier against the generic one")
    ap.add_argument("--routed", action="store_true", help="A/B of RSA routing (K20) off against on")
    ap.add_argument("--ab", nargs=3, default=None, metavar=("A.so", "A2.so", "B.so"),
                    help="the routing-off dense call through three libraries side by side")
    a = ap.parse_args()
    if a.keyed:
        return keyed_main(a)
    if a.routed:
        return routed_main(a)
    if a.ab:
        return ab_main(a)

    import torch
    if not torch.cuda.is_available():
        print("rsa_bench.py: no GPU", file=sys.stderr)
        return 2
    import bc_rsa_pss as bc
    from corda_amd.engine import Engine

    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        g = json.load(f)
    keys = []
    for k in g["keys"]:
        if "d" in k and int(k["e"], 16) == 65537 and 2048 < int(k["n"], 16).bit_length() <= 3072:
            keys.append({f: int(k[f], 16) for f in ("n", "e", "d", "p", "q")})
    try:
        import openssl_rsa_pss as ossl
        for _ in range(2):  # a handful of keys: two more from OpenSSL where it loads
            h, k = ossl.keygen(3072)
            ossl.free_key(h)
            keys.append(k)
    except (OSError, AttributeError, AssertionError) as exc:
        ossl = None
        ossl_error = str(exc)
    rng = random.Random(0xBE7C)
    n = 1 << a.rows_log2
    dist = []
    for i in range(a.distinct):
        k = keys[i % len(keys)]
        m = rng.randbytes(32)
        em = bc.encode_em(m, k["n"].bit_length(), rng.randbytes(32))
        sig = bc.sign_crt(em, k["p"], k["q"], k["d"]).to_bytes((k["n"].bit_length() + 7) // 8, "big")
        dist.append((k, sig, m))
    mod = np.zeros((a.distinct, W), np.uint32)
    exp = np.zeros(a.distinct, np.uint32)
    sigs = np.zeros((a.distinct, 4 * W), np.uint8)
    sl = np.zeros(a.distinct, np.uint16)
    msgs = np.zeros((a.distinct, 32), np.uint8)
    words = np.zeros((a.distinct, W), np.uint32)
    for i, (k, sig, m) in enumerate(dist):
        mod[i] = np.frombuffer(k["n"].to_bytes(4 * W, "little"), "<u4")
        exp[i] = k["e"]
        sigs[i, :len(sig)] = np.frombuffer(sig, np.uint8)
        sl[i] = len(sig)
        msgs[i] = np.frombuffer(m, np.uint8)
        words[i] = np.frombuffer(int.from_bytes(sig, "big").to_bytes(4 * W, "little"), "<u4")
    idx = np.arange(n) % a.distinct
    bad = np.zeros(n, bool)
    bad[rng.sample(range(n), n // 100)] = True
    rows_sig = sigs[idx]
    rows_sig[bad, 100] ^= 0x10  # 1 % corrupted
    dev = torch.device("cuda:0")
    t = lambda x, ty: torch.from_numpy(np.ascontiguousarray(x).view(ty)).to(dev)  # noqa: E731
    tm, te, tw = t(mod[idx], np.int32), t(exp[idx], np.int32), t(words[idx], np.int32)
    ts, tl, tg = t(rows_sig, np.uint8), t(sl[idx], np.int16), t(msgs[idx], np.uint8)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    verdict = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev)
    out = torch.empty((n, W), dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    res = {"workload": "rsa_pss_verify_device", "rows": n, "modulus_bits": 3072, "mod_words": W,
           "distinct_signatures": a.distinct, "keys": len(keys), "corrupted_rows": int(bad.sum()),
           "steps": a.steps, "warmup": a.warmup}
    with Engine(1) as eng:
        def verify():
            eng.rsa_pss_verify_device(tm, te, ts, tl, tg, status, verdict, stream=stream)

        def modexp():
            eng.rsa_public_op_device(tm, te, tw, out, stream=stream)

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            stream.synchronize()
            ms = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return ms
        vms = timed(verify)
        got = status.cpu().numpy()
        assert int((got == 0).sum()) == n - int(bad.sum()) and (got[bad] == 1).all(), "wrong statuses"
        mms = timed(modexp)
        v, m = float(np.median(vms)), float(np.median(mms))
        macs = n * products(65537) * 2 * W * W
        res.update({"verify_ms": v, "verify_ms_min": min(vms), "verify_ms_max": max(vms), "modexp_ms": m,
                    "modexp_ms_min": min(mms), "modexp_ms_max": max(mms), "prep_check_ms": v - m,
                    "verifs_per_s": n / (v * 1e-3), "products_per_row": products(65537),
                    "limb_macs_per_row": products(65537) * 2 * W * W, "limb_macs_per_s": macs / (m * 1e-3),
                    "fraction_of_peak": macs / (m * 1e-3) / PEAK_LIMB_MACS, "peak_limb_macs_per_s": PEAK_LIMB_MACS})
        import bench
        res["clock"] = bench._clock_under_load(0, verify, stream.synchronize, v)
    # the same rows on the CPU: OpenSSL libcrypto on cpu-threads threads
    if ossl is None:
        res["cpu"] = {"error": "libcrypto did not load: " + ossl_error}
    else:
        per = max(1, a.cpu_rows // a.cpu_threads)
        work = []
        for th in range(a.cpu_threads):
            k, _, _ = dist[th % len(dist)]
            der = bc.encode_key(k["n"], k["e"])
            mine = np.nonzero(idx % len(keys) == th % len(keys))[0][:per]  # this thread's key's rows
            rows = [(bytes(rows_sig[r, :sl[idx[r]]]), bytes(msgs[idx[r]])) for r in mine]
            work.append((der, rows))
        counts = [0] * a.cpu_threads

        def run(th):
            counts[th] = ossl.verify_rows(*work[th])
        threads = [threading.Thread(target=run, args=(th,)) for th in range(a.cpu_threads)]
        t0 = time.perf_counter()
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        dt = time.perf_counter() - t0
        total = sum(len(w[1]) for w in work)
        res["cpu"] = {"threads": a.cpu_threads, "rows": total, "seconds": dt, "verifs_per_s": total / dt,
                      "verified": int(sum(counts)), "library": "OpenSSL libcrypto EVP_DigestVerify through ctypes"}
        res["gpu_over_cpu"] = res["verifs_per_s"] / res["cpu"]["verifs_per_s"]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
