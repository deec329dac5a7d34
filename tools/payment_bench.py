"""A validating notary's batch of cash payments (corda_amd.corpus.cash_payment_items), wholly
device-resident, the one-stream step of K22 against what a caller does today, alternating in
one process, each round on a fresh commit log:

  (b) signed_txcomp_verify_ed25519_device -> txcomp_inputs_device -> commit_inputs_device ->
      ed25519_sign_keyed_device: the commit rows come out of the component items in HBM;
  (a) the same verify, commit and sign calls, but the refs, their offsets and the windows are the
      caller's own arrays, copied from (pinned) host memory on the same stream between verify and
      commit -- nothing ties them to the components that were hashed.

Figures are device ms between two events on the stream (the host-to-device copies of (a)
included), per batch of `--ntx` payments: median, min and max of `--steps` alternating rounds
after `--warmup`; `inputs_ms` is cordahip_last_kernel_ms of cordahip_txcomp_inputs_device
alone. Statuses, committed flags and notary signatures of (a) and (b) must be identical on
every transaction of every timed round (asserted). One JSON line.

  python tools/payment_bench.py --out profiles/r28_payment.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntx", type=int, default=1 << 16)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from corda_amd import _lib
    from corda_amd.corpus import cash_payment_items
    from corda_amd.engine import Engine

    n, nkeys = a.ntx, 256
    dev = torch.device("cuda", 0)
    now_s = 1500000000
    now, tol = now_s * 10**9, 60 * 10**9
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    with Engine(1) as eng:
        g = torch.Generator(device=dev)
        g.manual_seed(28)
        seeds = torch.randint(0, 256, (nkeys + 1, 32), dtype=torch.uint8, device=dev, generator=g)
        pubs, scratch = z(nkeys + 1, 32), z(nkeys + 1, 64)
        eng.ed25519_sign_device(seeds, z(nkeys + 1, 32), pubs, scratch)
        torch.cuda.synchronize(dev)
        pubs_h = pubs.cpu().numpy()
        c = cash_payment_items(pubs_h[:nkeys], pubs_h[nkeys].tobytes(), n, 28, now_s=now_s)
        # the owners' signatures over the ids, made by the device signer
        signer = np.concatenate([np.asarray(sg, np.int64) for sg in c["signers"]])
        tso = np.zeros(n + 1, np.int64)
        tso[1:] = np.cumsum([len(sg) for sg in c["signers"]])
        nsig = len(signer)
        sig_tx = np.repeat(np.arange(n), np.diff(tso))
        d_ids = up(c["ids"])
        d_keys, d_sigs = z(nsig, 32), z(nsig, 64)
        eng.ed25519_sign_device(seeds[up(signer)].contiguous(), d_ids[up(sig_tx)].contiguous(), d_keys, d_sigs)
        torch.cuda.synchronize(dev)
        key_id, _ = eng.signer_add_ed25519(seeds[nkeys].cpu().numpy().tobytes())

        items, n_items = c["items"], len(c["items"])
        d_items = up(items.view(np.uint8).reshape(-1, _lib.KRYO_ITEM_DTYPE.itemsize))
        d_blob, d_tio, d_tso = up(c["blob"]), up(c["tx_item_off"].astype(np.int64)), up(tso)
        d_caller = up(np.ones(n, np.int32))
        d_key_id = torch.full((n,), key_id, dtype=torch.int32, device=dev)
        # (a)'s separate arrays, as a caller holds them: pinned host memory
        refs_h = np.zeros(sum(len(r) for r in c["refs"]), _lib.STATE_REF_DTYPE)
        flat = [r for rs in c["refs"] for r in rs]
        refs_h["txhash"] = np.frombuffer(b"".join(h for h, _ in flat), np.uint8).reshape(-1, 32)
        refs_h["index"] = [i for _, i in flat]
        n_refs = len(refs_h)
        ro_h = np.zeros(n + 1, np.int64)
        ro_h[1:] = np.cumsum([len(r) for r in c["refs"]])
        side = lambda w, k: _lib.TW_SIDE_ABSENT if w is None or w[k] is None else w[k][0] * 10**9 + w[k][1]  # noqa: E731
        twf_h = np.array([side(w, 0) for w in c["windows"]], np.int64)
        twu_h = np.array([side(w, 1) for w in c["windows"]], np.int64)
        pin = lambda x: torch.from_numpy(np.ascontiguousarray(x)).pin_memory()  # noqa: E731
        p_refs, p_ro, p_twf, p_twu = pin(refs_h.view(np.uint8).reshape(-1, 36)), pin(ro_h), pin(twf_h), pin(twu_h)

        def outputs():
            return dict(txid=z(n, 32), vst=z(n), fb=z(n, dt=torch.int64), sst=z(nsig), refs=z(n_refs, 36),
                        ro=z(n + 1, dt=torch.int64), twf=z(n, dt=torch.int64), twu=z(n, dt=torch.int64), gate=z(n),
                        cst=z(n), com=z(n), rst=z(n_refs), rby=z(n_refs, 40), nsig=z(n, 64), nst=z(n))

        oa, ob = outputs(), outputs()
        s = torch.cuda.Stream(dev)
        log2 = max(10, int(np.ceil(np.log2(n_refs * 8 / 7))) + 1)

        def verify(o):
            eng.signed_txcomp_verify_ed25519_device(d_items, n_items, d_blob, d_tio, d_tso, d_keys, d_sigs, o["txid"],
                                                    o["vst"], o["fb"], o["sst"], stream=s)

        def commit_and_sign(o, log, gate):
            eng.commit_inputs_device(log, o["txid"], d_caller, o["refs"], o["ro"], o["cst"], o["com"], o["rst"], o["rby"],
                                     o["twf"], o["twu"], now, tol, gate=gate, stream=s)
            eng.ed25519_sign_keyed_device(d_key_id, o["txid"], o["nsig"], o["nst"], gate=o["cst"], stream=s)

        def step_b(o, log):
            verify(o)
            eng.txcomp_inputs_device(d_items, n_items, d_blob, d_tio, o["refs"], o["ro"], o["twf"], o["twu"], o["gate"],
                                     tx_status=o["vst"], stream=s)
            commit_and_sign(o, log, o["gate"])

        def step_a(o, log):
            verify(o)
            with torch.cuda.stream(s):
                o["refs"].copy_(p_refs, non_blocking=True)
                o["ro"].copy_(p_ro, non_blocking=True)
                o["twf"].copy_(p_twf, non_blocking=True)
                o["twu"].copy_(p_twu, non_blocking=True)
            commit_and_sign(o, log, o["vst"])

        def timed(fn, o):
            log = eng.commit_log_create(log2)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fn(o, log)
            e1.record(s)
            s.synchronize()
            eng.commit_log_destroy(log)
            return e0.elapsed_time(e1)

        ta, tb, ti = [], [], []
        for step in range(a.warmup + a.steps):
            ms_a, ms_b = timed(step_a, oa), timed(step_b, ob)
            for k in ("txid", "vst", "sst", "refs", "ro", "twf", "twu", "cst", "com", "rst", "rby", "nsig", "nst"):
                assert torch.equal(oa[k], ob[k]), k
            assert not ob["gate"].any().item() and int(ob["com"].sum().item()) == n and not ob["nst"].any().item()
            eng.txcomp_inputs_device(d_items, n_items, d_blob, d_tio, ob["refs"], ob["ro"], ob["twf"], ob["twu"],
                                     ob["gate"], tx_status=ob["vst"], stream=s)
            s.synchronize()
            if step >= a.warmup:
                ta.append(ms_a)
                tb.append(ms_b)
                ti.append(eng.last_kernel_ms(0))
        eng.signer_remove(key_id)

    def fig(x):
        return {"median_ms": round(statistics.median(x), 3), "min_ms": round(min(x), 3), "max_ms": round(max(x), 3)}

    res = {"bench": "payment", "ntx": n, "items": int(n_items), "refs": int(n_refs), "signatures": int(nsig),
           "windows": int(sum(w is not None for w in c["windows"])), "payload_bytes": int(c["blob"].size),
           "steps": a.steps, "warmup": a.warmup, "txcomp_inputs_device_ms": fig(ti),
           "b_one_stream_step_device_ms": fig(tb), "a_refs_uploaded_from_host_device_ms": fig(ta),
           "bytes_h2d_separate_arrays_per_tx": round((refs_h.nbytes + ro_h.nbytes + twf_h.nbytes + twu_h.nbytes) / n, 1),
           "outputs_identical": True}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
