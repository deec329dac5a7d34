"""RSA_SHA256 signing with registered private keys on one GPU: the keyed signer (K19,
cordahip_rsa_sign_keyed_device) over rows resident in HBM, 32-byte messages and salts, against
the keyed verifier (K18, cordahip_rsa_verify_keyed_device) over exactly the signatures it
produced, in ONE process, the two alternating step by step so that both see the same machine.
Device events around each launch on the workload's stream. Prints ONE JSON line; per leg (one
2048-bit key, one 3072-bit key, one 4096-bit key, and the mixed 3072-bit-class keys of
tools/rsa_bench.py -- the fixture's e = 65537 keys of that class and, where the local libcrypto
loads, two more from OpenSSL; lane i signs with key i mod K):
  sign_ms, verify_ms       median step of each (min / max beside them), *_per_s
  rejected                 lanes whose signing status is not OK plus lanes K18 does not accept; must be 0
  ratio_measured           sign_ms / verify_ms
  ratio_model              the product-count model's: half-width Montgomery products at a quarter of a
                           full-width one -- per half exponentiation windows * (w + 1) products, the
                           table's 2^w - 1 and two for the reduction; three for the recombination; one
                           full-width product for q h and the fault check's chain -- over K18's chain
  clock                    shader clock sampled beside one extra untimed signing step
The run fails unless every produced signature verifies. A run without a GPU fails; nothing falls
back. --lib loads another build of the library (an A/B variant of the window width or the block
size, built with -DCORDAHIP_RSA_SIGN_WIN / -DCORDAHIP_RSA_SIGN_BLOCK) and --window states its
window width for the model; --sign-only skips the verifier's steps.
  python tools/rsa_sign_bench.py [--rows-log2 16] [--steps 5] [--warmup 1] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def chain_products(e):
    """K18's chain: a square per bit below the top one, a multiply per set one among them, the product with K"""
    return (e.bit_length() - 1) + (bin(e).count("1") - 1) + 1


def model(bits_p, w, e):
    """(signing in full-width product equivalents, K18's products) for primes of bits_p bits"""
    nwin = (32 * ((bits_p + 31) // 32) + w - 1) // w
    half = 2 * (nwin * (w + 1) + (1 << w) - 1 + 2) + 3
    return half / 4.0 + 1 + chain_products(e), chain_products(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-log2", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", nargs="+", default=["2048", "3072", "4096", "mixed3072"])
    ap.add_argument("--lib", default=None)
    ap.add_argument("--variant", default="shipped")
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--sign-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("rsa_sign_bench.py: no GPU", file=sys.stderr)
        return 2
    import bench
    import bc_rsa_pss as bc
    from corda_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from corda_amd.engine import Engine

    with open(os.path.join(ROOT, "tests", "golden", "rsa_pss_vectors.json")) as f:
        g = json.load(f)
    fix = [{f: int(k[f], 16) for f in ("n", "e", "d", "p", "q")} for k in g["keys"] if "d" in k and int(k["e"], 16) == 65537]
    mixed = [k for k in fix if 2048 < k["n"].bit_length() <= 3072]
    try:
        import openssl_rsa_pss as ossl
        for _ in range(2):
            h, k = ossl.keygen(3072)
            ossl.free_key(h)
            mixed.append(k)
    except (OSError, AttributeError, AssertionError):
        pass
    one = lambda bits: [k for k in fix if k["n"].bit_length() == bits][:1]  # noqa: E731
    legs = {"2048": ("one 2048-bit key", 64, one(2048)), "3072": ("one 3072-bit key", 96, one(3072)),
            "4096": ("one 4096-bit key", 128, one(4096)), "mixed3072": ("mixed 3072-bit-class keys", 96, mixed)}

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    n = 1 << a.rows_log2
    res = {"workload": "rsa_sign_keyed_device against rsa_verify_keyed_device over its signatures, alternating; "
                       "32-byte messages and salts in HBM",
           "variant": a.variant, "window": a.window, "rows": n, "steps": a.steps, "warmup": a.warmup, "legs": []}
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
        gen.manual_seed(0x5173)
        msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        salts = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        for leg in a.legs:
            name, w, keys = legs[leg]
            assert keys, name
            sids, vids = [], []
            for k in keys:
                p, q = k["p"], k["q"]
                kid, st, mod = eng.signer_add_rsa(p, q, k["d"] % (p - 1), k["d"] % (q - 1), pow(q, -1, p), k["e"])
                assert st == 0 and int.from_bytes(mod, "big") == k["n"]
                vid, vst = eng.vkey_add_rsa(bc.encode_key(k["n"], k["e"]))
                assert vst == 0
                sids.append(kid)
                vids.append(vid)
            lane_key = torch.arange(n, device=dev) % len(keys)
            t_sid = torch.from_numpy(np.array(sids, np.uint32).view(np.int32).copy()).to(dev)[lane_key].contiguous()
            t_vid = torch.from_numpy(np.array(vids, np.uint32).view(np.int32).copy()).to(dev)[lane_key].contiguous()
            sig = torch.empty((n, 4 * w), dtype=torch.uint8, device=dev)
            slen = torch.empty(n, dtype=torch.int16, device=dev)
            sst = torch.empty(n, dtype=torch.uint8, device=dev)
            vst_t = torch.zeros(n, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)

            def sign():
                eng.rsa_sign_keyed_device(t_sid, msgs, salts, sig, slen, sst, stream=stream)

            def verify():
                eng.rsa_verify_keyed_device(t_vid, sig, slen, msgs, vst_t, stream=stream)

            both = [("sign", sign)] + ([] if a.sign_only else [("verify", verify)])
            for _ in range(a.warmup):
                for _, fn in both:
                    fn()
            stream.synchronize()
            ms = {nm: [] for nm, _ in both}
            for _ in range(a.steps):  # alternating: both see the same machine
                for nm, fn in both:
                    ms[nm].append(timed(fn))
            rejected = int((sst != 0).sum()) + int((vst_t != 0).sum())
            bad += rejected
            run = {"leg": name, "mod_words": w, "keys": len(keys), "rejected": rejected}
            for nm, _ in both:
                m = float(np.median(ms[nm]))
                run.update({nm + "_ms": m, nm + "_ms_min": min(ms[nm]), nm + "_ms_max": max(ms[nm]),
                            nm + "_per_s": n / (m * 1e-3)})
            # the leg's model is its first key's: the mixed leg's keys share e, and their prime
            # lengths round to the same number of exponent words, so to the same window count
            k0 = keys[0]
            eq, ver = model(max(k0["p"].bit_length(), k0["q"].bit_length()), a.window, k0["e"])
            run.update({"sign_full_width_equivalents": eq, "verify_products": ver, "ratio_model": eq / ver})
            if not a.sign_only:
                run["ratio_measured"] = run["sign_ms"] / run["verify_ms"]
                run["measured_over_model"] = run["ratio_measured"] / run["ratio_model"]
            run["clock"] = bench._clock_under_load(0, sign, stream.synchronize, run["sign_ms"])
            res["legs"].append(run)
            for kid in sids:
                eng.signer_remove(kid)
            for vid in vids:
                eng.vkey_remove(vid)
    res["rejected"] = bad
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
