"""Run by tests/test_gpu_ecdsa_sign.py in a fresh process with CORDAHIP_HOST_CHUNK=256: 700 lanes of mixed
message lengths through cordahip_ecdsa_sign_submit, two tickets outstanding (three chunks each: 256, 256,
188 lanes; dense 32-byte chunks and CSR ones), every row compared with the device call's over the same
lanes and a sample with the model. Prints one JSON line."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ecdsa_sign_model as M  # noqa: E402


def main():
    import torch
    from corda_amd.engine import Engine
    g = json.load(open(os.path.join(HERE, "golden", "ecdsa_sign_vectors.json")))
    n = 700
    lens = [32 if i < 256 else (1, 31, 32, 33, 55, 64, 120, 200)[i % 8] for i in range(n)]
    ok, with_device, with_model = True, 0, 0
    with Engine(1) as eng:
        keys = []
        for k in g["keys"]:
            kid, st, pub = eng.signer_add_ecdsa(k["scheme"], bytes.fromhex(k["d"]))
            ok &= st == 0 and pub.hex() == k["pub"]
            keys.append((kid, k["scheme"], int(k["d"], 16)))
        batches = []
        for b in range(2):
            who = [keys[(i + 3 * b) % len(keys)] for i in range(n)]
            msgs = [hashlib.shake_256(b"ecdsa-chunk-%d-%d" % (b, i)).digest(lens[i]) for i in range(n)]
            batches.append((who, msgs, eng.ecdsa_sign_batch([w[0] for w in who], msgs, async_=True)))
        dev = torch.device("cuda:0")
        for who, msgs, ticket in batches:
            sig, ln, st = ticket.wait()
            ok &= not st.any()
            for L in sorted(set(lens)):  # the device call takes dense rows: one call per length
                sel = [i for i in range(n) if lens[i] == L]
                t_ids = torch.from_numpy(np.asarray([who[i][0] for i in sel], np.uint32).view(np.int32).copy()).to(dev)
                t_msg = torch.from_numpy(np.frombuffer(b"".join(msgs[i] for i in sel), np.uint8)
                                         .reshape(len(sel), L).copy()).to(dev)
                t_sig = torch.full((len(sel), 72), 0xA5, dtype=torch.uint8, device=dev)
                t_len = torch.full((len(sel),), 0xA5, dtype=torch.uint8, device=dev)
                t_st = torch.full((len(sel),), 0xA5, dtype=torch.uint8, device=dev)
                eng.ecdsa_sign_keyed_device(t_ids, t_msg, t_sig, t_len, t_st)
                torch.cuda.synchronize()
                ok &= not t_st.cpu().numpy().any()
                ok &= np.array_equal(t_sig.cpu().numpy(), sig[sel]) and np.array_equal(t_len.cpu().numpy(), ln[sel])
                with_device += len(sel)
            for i in range(0, n, 50):
                want = M.sign(M.CURVES[who[i][1]], who[i][2], msgs[i])
                ok &= int(ln[i]) == len(want) and sig[i].tobytes() == want + bytes(72 - len(want))
                with_model += 1
    print(json.dumps({"ok": bool(ok), "lanes": n, "tickets": len(batches), "chunk": os.environ.get("CORDAHIP_HOST_CHUNK"),
                      "compared_with_device": with_device, "compared_with_model": with_model}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
